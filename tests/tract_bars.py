"""Bars of the tract-posterior tests (tests/test_tracts.py), in one place: 5 x the largest error measured on the MI355X over the
grid of test_tracts_against_the_oracle (K = 4, 8, 12 padded, 16, 32, 64; both parameter layouts; W = 0 / 37; bins 1 / 7 / 100;
ragged lens; a prefix set, an interior set and fractional weights), the project's rule (tests/parity_bars.py).

``tract``: largest absolute error of the tract probabilities against the float64 dense oracle.
"""

F32_TRACT_BAR = 1.9e-5  # measured worst 3.72e-6 (K = 8; K = 4: 2.4e-6, 12: 1.4e-6, 16: 1.8e-6, 32: 8.3e-7, 64: 1.1e-6)
F64_TRACT_BAR = 3.1e-14  # measured worst 6.11e-15 (K = 8; K = 4: 5.1e-15, 12: 3.0e-15, 16: 3.3e-15, 32: 2.3e-15, 64: 2.9e-15)

# bin = 1 against sum_k m(k) gamma_t(k) from phk_posterior's marginals (K = 16, 3 particles x 4 rows x 4,800 sites, the grid's
# three weight rows): 5 x the measured worst
F32_MARGINAL_BAR = 2.1e-6  # measured worst 4.14e-7
F64_MARGINAL_BAR = 4.5e-15  # measured worst 8.88e-16

# log of one bin over a whole row against ll(emis0, emis1 multiplied by m) - ll from the shipped no-gradient call, float64,
# K = 16, 2 particles x 2 rows of 200 sites (log tract -5.2 .. -8.3): 5 x the measured 2.31e-14
F64_LIKELIHOOD_RATIO_BAR = 1.2e-13

# the structured float64 statement (tests/tract_oracle.structured) against the dense oracle on the GPU grid's inputs (every
# particle and row, both layouts, the grid's weights, bins and lens) in the grid's own metric, measured on the CPU: the float64
# rounding floor of the kernel's form.  The float64 bar above must stay within 10 x it; the statement itself is held to 5 x it.
# (The dense oracle's matrix products go through the host's BLAS, so the figure moves a little between hosts -- 6.4e-15 at K = 8 on
# another -- which is what the 5 x is for; the smaller figure is kept, as the stricter one for the float64 bar.)
STRUCTURED_FLOOR = 6.106e-15  # K = 8 (K = 4: 5.8e-15, 12: 2.8e-15, 16: 5.1e-15, 32: 2.3e-15, 64: 1.9e-15)
STRUCTURED_FLOOR_BAR = 5 * STRUCTURED_FLOOR
