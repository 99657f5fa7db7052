"""Bars of the interval-tract tests (tests/test_interval_tracts.py), in one place: 5 x the largest error measured on the MI355X
against the float64 oracle (tests/interval_oracle.py), the project's rule (tests/parity_bars.py).

The metric is |logp - oracle| / max(1, |oracle|): absolute for a probable segment, relative for an improbable one.
"""

# the grid of test_intervals_against_the_oracle (K = 4, 8, 12 padded, 16, 32, 64; both parameter layouts; W = 0 / 37; a list per
# row with length-1, adjacent, block-crossing and row-ending intervals; shared and per-particle sets)
F32_GRID_BAR = 1e-5  # the project's cap; measured worst 3.92e-6 (K = 8; K = 4: 1.0e-6, 12: 2.1e-6, 16: 1.8e-6, 32: 1.2e-6, 64: 1.4e-6): 5 x it is above the cap
F64_GRID_BAR = 8.4e-14  # measured worst 1.68e-14 (K = 8; K = 4: 1.3e-14, 12: 5.3e-15, 16: 4.2e-15, 32: 4.1e-15, 64: 5.9e-15)

# one interval of 4,000 windows, K = 16 float32, an interior set (test_a_tract_below_the_float_range_is_right_as_a_log)
F32_LONG_BAR = 3.5e-6  # measured 6.90e-7 (logp -140 .. -222; 2.4e-8 per window)

# log(tract_oracle.structured) -- the kernel's recursion in float64 loops -- against the interval oracle on regular intervals of 7
# and 100 positions of the grid's rows (both layouts, a prefix and an interior set), in the metric above, measured on the CPU: the
# float64 rounding floor of the kernel's form.  The float64 bar above must stay within 10 x it.
STRUCTURED_FLOOR = 2.234e-14  # K = 4 (K = 8: 1.5e-14, 12: 1.6e-14, 16: 2.1e-14, 32: 9.3e-15, 64: 8.1e-15)
STRUCTURED_FLOOR_BAR = 5 * STRUCTURED_FLOOR
