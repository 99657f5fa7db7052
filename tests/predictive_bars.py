"""Bars of the leave-one-out predictive tests (tests/test_predictive.py), in one place: 5 x the largest error measured on the
MI355X over the grid of test_predictive_against_the_oracle (K = 4, 8, 12 padded, 16, 32, 64; both parameter layouts; W = 0 / 37;
bins 1 / 7 / 100; ragged lens), the project's rule (tests/parity_bars.py).

``het``: largest absolute error of the bin sums of phet (over the observed and over the missing sites) against the float64
dense oracle.
``score``: largest error of the bin sums of the log score relative to max(1, |oracle|).
"""

F32_HET_BAR = 4.0e-5  # measured worst 7.92e-6 (K = 8)
F64_HET_BAR = 6.7e-14  # measured worst 1.33e-14 (K = 8)
F32_SCORE_BAR = 7.8e-6  # measured worst 1.56e-6 (K = 32)
F64_SCORE_BAR = 1.7e-14  # measured worst 3.33e-15 (K = 8)

# phet at nine probe sites of one row against 1 / (1 + exp(ll_hom - ll_het)) from the shipped no-gradient call, float64, K = 16:
# 5 x the measured 4.58e-16 (site 16; the probes inside the missing run and at the isolated missing site 4.1e-16 and 4.2e-16)
F64_LIKELIHOOD_RATIO_BAR = 2.3e-15

# the structured float64 statement (tests/predictive_oracle.structured) against the dense oracle on the GPU grid's inputs (every
# particle and row, both layouts) in the grid's own metric, measured on the CPU: the float64 rounding floor of the kernel's form.
# The float64 bars above must stay within 10 x these; the statement itself is held to 5 x them.
STRUCTURED_HET_FLOOR = 1.155e-14  # K = 8 (K = 4: 4.4e-16, 12: 5.3e-15, 16: 4.0e-15, 32 and 64: 4.4e-15)
STRUCTURED_SCORE_FLOOR = 3.664e-15  # K = 8 (K = 4: 7.8e-16, 12: 1.1e-15, 16: 1.3e-15, 32: 2.0e-15, 64: 1.1e-15)
STRUCTURED_HET_FLOOR_BAR = 5 * STRUCTURED_HET_FLOOR
STRUCTURED_SCORE_FLOOR_BAR = 5 * STRUCTURED_SCORE_FLOOR
