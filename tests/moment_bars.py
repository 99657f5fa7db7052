"""Bars of the bin-moment tests (tests/test_bin_moments.py), in one place, each beside the figure it was derived from.

Metrics of the oracle grid (test_moments_against_the_oracle: K = 4, 8, 12 padded, 16, 32, 64; both parameter layouts; W = 0 / 37;
bins 1 / 7 / 100; the ragged lens of test_tracts.grid_sets(); a centred monotone row per particle, an indicator and a shared
random signed row): ``m1`` = max |m1 - oracle| / max(1, |oracle|), ``m2`` = max |m2 - oracle| / max(1, oracle), against the float64
dense oracle (tests/moment_oracle.dense).  The larger of the two is held to the bar.
"""

# float32, per K: 5 x the largest error measured on the MI355X (the rule of tests/parity_bars.py)
F32_MEASURED = {  # K: (m1, m2)
    4: (1.719e-06, 2.106e-06),
    8: (6.412e-05, 9.207e-06),
    12: (1.965e-04, 5.670e-06),
    16: (6.426e-06, 7.079e-06),
    32: (5.412e-05, 7.690e-06),
    64: (4.268e-05, 3.717e-06),
}
F32_MOMENT_BAR = {K: 5 * max(m) for K, m in F32_MEASURED.items()}

# the structured float64 statement (tests/moment_oracle.structured) against the dense oracle on the GPU grid's inputs (every
# particle and row, both layouts, the grid's value rows, bins and lens) in the grid's own metrics, measured on the CPU: the
# float64 rounding floor of the kernel's form.  The statement itself is held to 5 x it (the dense oracle's matrix products go
# through the host's BLAS, so the figure moves a little between hosts); the float64 GPU bar is 10 x it.
STRUCTURED_MEASURED = {  # K: (m1, m2)
    4: (5.035e-15, 4.201e-15),
    8: (9.870e-14, 1.499e-14),
    12: (2.861e-13, 1.007e-14),
    16: (1.723e-14, 1.726e-14),
    32: (1.866e-13, 1.038e-14),
    64: (1.276e-13, 8.222e-15),
}
STRUCTURED_FLOOR = max(max(m) for m in STRUCTURED_MEASURED.values())
STRUCTURED_FLOOR_BAR = 5 * STRUCTURED_FLOOR
F64_MOMENT_BAR = 10 * STRUCTURED_FLOOR
F64_MEASURED = 2.954e-13  # (m1, K = 12) the largest float64 error measured on the MI355X over the grid, either metric (for the record: the bar is the line above)

# The cumulant identity K(h) = log E[exp(h S) | o] through the tract oracle at h = 1e-4 (test_cumulant_identity_through_the_tract_oracle:
# L = 700, bins 7 and 100, K = 4 and 16, a monotone row in [0, 1]): (K(h) - K(-h)) / 2h against m1 in units of max(1, |m1|),
# (K(h) + K(-h)) / h^2 against the variance in units of max(1, var).  Measured on the CPU, float64 oracles on both sides: the
# truncation of the central differences plus the rounding of the differenced logs.  Bars: 10 x.
CUMULANT_H = 1e-4
CUMULANT_M1_MEASURED = 3.211e-9  # K = 16, bin = 100 (K = 4: 5.9e-11 at bin 7, 6.6e-10 at bin 100; K = 16, bin 7: 2.3e-11)
CUMULANT_VAR_MEASURED = 7.501e-7  # K = 4, bin = 100 (K = 4, bin 7: 1.8e-7; K = 16: 1.5e-7 at bin 7, 4.1e-8 at bin 100)
CUMULANT_M1_BAR = 10 * CUMULANT_M1_MEASURED
CUMULANT_VAR_BAR = 10 * CUMULANT_VAR_MEASURED

# tmrca_band's mean against posterior_tmrca at the same bin (two contigs, three models, float32, K = 16), relative to the
# largest value of the track: 5 x the difference measured on the MI355X
BAND_MEAN_MEASURED = 8.325e-8
BAND_MEAN_BAR = 5 * BAND_MEAN_MEASURED
