"""Bars of the local likelihood-ratio tests (tests/test_local_ratio.py), in one place, by the project's rule
(tests/parity_bars.py): a float32 bar is at most 5 x the largest error measured on the MI355X, the float64 bar is 10 x the
rounding floor of the kernel's own form measured on the CPU.

The grid's metric is |log ratio - oracle| / max(1, |oracle|) against the float64 dense oracle (tests/local_oracle.dense), over
the grid of test_local_ratio_against_the_oracle (K = 4, 8, 12 padded, 16, 32, 64; both parameter layouts; W = 0 / 37; bins
1 / 7 / 100; ragged lens; theta x 4 as one block, rho / 4 and Ne x 2 with a block per model).
"""

# the structured float64 statement (tests/local_oracle.structured) against the dense oracle on the GPU grid's inputs (every
# particle and row, both layouts, the grid's alternatives, bins and lens) in the grid's own metric, measured on the CPU: the
# float64 rounding floor of the kernel's form.  The statement itself is held to 5 x it (the dense oracle's matrix products go
# through the host's BLAS, so the figure moves a little between hosts).
STRUCTURED_FLOOR = 1.543e-14  # K = 16 (K = 4: 1.48e-14, 8: 1.29e-14, 12: 1.41e-14, 32: 7.4e-15, 64: 7.4e-15)
STRUCTURED_FLOOR_BAR = 5 * STRUCTURED_FLOOR

# the grid; also the plans (serial, segmented) x rescale intervals (1, 2, 4) at K = 16, which measured 6.21e-6 / 1.16e-14
# everywhere, and the range test (log ratios of 77 .. 851: 7.8e-8 / 1.1e-15)
F32_LOCAL_BAR = 3.9e-5  # measured worst 7.96e-6 (K = 4; K = 8: 6.9e-6, 12: 5.6e-6, 16: 6.2e-6, 32: 5.5e-6, 64: 3.2e-6)
F64_LOCAL_BAR = 10 * STRUCTURED_FLOOR  # measured worst 1.62e-14 (K = 8; K = 4: 1.5e-14, 12: 1.3e-14, 16: 1.1e-14, 32: 9.6e-15, 64: 9.7e-15)

# one bin over a whole row against ll(alternative fields with the fitted pi) - ll from the shipped no-gradient call, float64,
# K = 16, 2 particles x 2 rows of 200 sites, absolute: 5 x the measured 8.88e-15
F64_LIKELIHOOD_RATIO_BAR = 4.4e-14

# emissions multiplied by an indicator on rows without missing windows: |exp(log ratio) - PSMCKernel.tracts' probability|,
# K = 16, 3 particles x 3 rows of 900 sites, bins 1 / 7 / 100.  float32: 5 x the measured 2.66e-8.  float64: measured 4.2e-17,
# below the spacing of the numbers compared; the bar is that of the tract sweep itself (tests/tract_bars.F64_TRACT_BAR), which
# runs the same operations up to the log and the exp.
F32_TRACT_CASE_BAR = 1.3e-7
F64_TRACT_CASE_BAR = 3.1e-14

# emissions set to 1 at bin = 1 against minus PSMCKernel.predictive's leave-one-out score, |sum| / max(1, |score|), K = 16,
# 3 particles x 4 rows x 4,800 scored sites: 5 x the measured 4.51e-7 / 8.22e-16
F32_BLOCK_OUT_BAR = 2.2e-6
F64_BLOCK_OUT_BAR = 4.1e-15
