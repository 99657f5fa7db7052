"""Seeded random draws over PARTICLE space for the sampler-side kernels (``phk_param_map``, ``phk_log_prior``, ``phk_chain_rule``,
``phk_svgd_step``), in the style of tests/model_fuzz.py.  Test infrastructure only, CPU only: numpy and ``oracle.psmc_numpy``
(``oracle.psmc_torch`` for the second opinion of the admission rule), nothing from ``phlash_amd``.  Used by
tests/test_sampler_fuzz.py.

Part A, the particle map.  ``param_map_kernel`` has about a dozen data-dependent branches ("Sampler-side fuzz"); a case
is a batch of 3 ... 9 particles of which one to three are pushed into a regime that reaches some of them, the rest staying
ordinary (a wrong particle offset shows).  Half of the cases are plain wide populations instead.  The map is discontinuous at
its branch thresholds and the two oracles themselves part there, so a case is admitted only if the branch predicates of every
particle are unchanged under +-1e-6 on every coordinate and the two oracles agree on it to 1e-11 row-scaled; a rejected case is
redrawn from the next sub-seed.  The predicates are computed from the oracle's own functions (``branch_state``).
``mp_block`` is the same map in 60-digit arithmetic (mpmath): the yardstick for the float64 references' own error.

Part B, the SVGD / AMSGrad step.  ``svgd_reference`` is a vectorised ``np.longdouble`` statement of the update with forward-error
bounds from absolute sums; ``select_population`` builds the populations whose pairwise distances drive the bucket select.

``draw_map(seed)``, ``draw_update(seed)`` are deterministic and return plain numpy.
"""

from __future__ import annotations

import functools
import math
import types

import numpy as np

from oracle import psmc_numpy as pn

# ------------------------------------------------------------------------------------------------- part A: the draw
KS = (5, 7, 16, 32, 64)
K_CYCLE = (5, 7, 16, 32, 64, 7, 16, 5, 32, 16)  # by seed mod 10: K = 64 once, where the autograd reference costs most
# 16 / 32 / 64: the patterns of tests/test_above_the_scan.py; 5 and 7: an epoch that covers the first state and another that covers
# the last state only -- the smallest sizes that still run every k == 0, k == 1 and last special case of the kernel
PATTERNS = {5: "2+2+1", 7: "3+1+2+1", 16: "14*1+1*2", 32: "30*1+1*2", 64: "4+25*2+4+6"}
THETAS = (1e-2, 1e-4)
LO, P_LO, P_HI = 1e-20, 1e-8, 1.0 - 1e-8
PERTURB = 1e-6  # the admission rule's step on every coordinate
ORACLES_AGREE = 1e-11  # ... and its bar on the two oracles, row-scaled
# single regimes: name -> (coordinate, value); coordinate "first" / "mid" / "last" / "any" = a c_tr of that epoch ("any": not the last)
SINGLES = (
    ("c25-first", "first", 25.0), ("c25-mid", "mid", 25.0), ("c25-last", "last", 25.0),
    ("c120-first", "first", 120.0), ("c120-mid", "mid", 120.0), ("c120-last", "last", 120.0),
    ("c-19-any", "any", -19.0), ("c-19-last", "last", -19.0),
    ("t1-20", "t1", -20.0), ("t1-30", "t1", -30.0), ("tM6", "tM", 6.0), ("rho40", "rho", 40.0), ("rho-40", "rho", -40.0),
)
# (log t1 = -50 is not among them: below t1 ~ 1e-16 the first states' E[t] = 1 / c + t - dt / expm1(c dt) is a rounding residue, 0 or a
# multiple of 2^-53, so whether the 1e-20 floor acts flips under +-1e-6 and between the two oracles; the admission rule rejected more
# than half of such draws.  The floor is reached robustly through c > 100 in the first epoch, where E[t_0] = t_0 = 0.)
# tags every one of which must come up (tests/test_sampler_fuzz.py states how often)
BRANCH_TAGS = ("softplus>20", "c>100", "c~0", "skip-dt", "series-u", "e-floor", "expm1inv>10", "emis0-lo", "emis1-lo", "b-lo",
               "pi-lo", "p2-lo", "p3-lo", "p3-hi", "A0k-lo")


def epoch_of_state(pat):
    return np.array([e for e, w in enumerate(pn.parse_pattern(pat)) for _ in range(w)], dtype=np.int32)


def row_scaled(got, want):
    """max over rows of |got - want| / max|row of want| for [..., 7, K] blocks: the metric of tests/test_above_the_scan.py"""
    scale = np.abs(want).max(-1, keepdims=True)
    return float((np.abs(got - want) / np.where(scale > 0, scale, 1.0)).max())


def branch_state(x, pat, theta):
    """What ``param_map_kernel`` branches on for one particle, from the oracle's own functions: -> dict name -> bool array (one
    entry per epoch / state / interval of the augmented grid)."""
    dm = pn.particle_to_dm(x, pat, theta)
    t, c, rho = np.asarray(dm.t), np.asarray(dm.c), dm.rho
    M = len(t)
    P = len(pn.parse_pattern(pat))
    e = pn.ect(t, c)
    ck, dt = c[:-1], np.diff(t)
    p = {}
    p["softplus>20"] = np.asarray(x[2:2 + P]) > 20.0
    p["c~0"] = np.isclose(ck, 0.0)
    p["c>100"] = np.isinf(ck) | (ck > 100.0)
    p["expm1inv>10"] = ~p["c~0"] & ~p["c>100"] & (ck * dt > 10.0)
    p["e-floor"] = e == LO  # (ect returns max(., 1e-20))
    # the augmented grid [t0, e0, t1, e1, ...] (transition.py:43) and row 0 of the running products
    t_aug = np.stack([t, e], 1).reshape(-1)
    dta = np.diff(t_aug)
    cr = np.repeat(c, 2)[:-1]
    skip = np.isclose(dta, 0.0)
    r_, c_ = 2.0 * dta * rho, dta * cr
    u = np.sqrt((2.0 * c_) ** 2 + r_ * r_) / 2.0  # expQ's u at n = 2
    p["skip"] = skip
    p["series-u"] = ~skip & (u < 1e-6)
    caused = np.zeros_like(skip)
    caused[0:2 * (M - 1):2] = p["c>100"]  # t_k -> e_k = t_k is the skip the c > 100 branch itself makes
    p["skip-dt"] = skip & ~caused
    rows = [np.array([1.0, 0.0, 0.0])]
    for k in range(2 * M - 1):
        rows.append(rows[-1] if skip[k] else rows[-1] @ pn.expQ(float(r_[k]), float(c_[k]), 2))
    R_t, R_e = rows[0::2], rows[1::2]  # at t_0 .. t_{M-1};  at e_0 .. e_{M-1}
    b = np.array([R_t[j + 1][2] - R_t[j][2] for j in range(M - 1)])
    gap = (t[1:] - e[:-1]) * ck
    q = np.concatenate([-np.expm1(-gap), [1.0]])
    d = np.array([R_e[j][0] + R_e[j][1] * q[j] + R_e[j][2] - R_t[j][2] for j in range(M)])
    p1 = np.array([R_e[j][1] for j in range(M)]) * np.concatenate([np.exp(-gap), [0.0]])
    p2 = np.concatenate([np.exp(-dt * ck), [0.0]])
    p3 = np.concatenate([-np.expm1(-dt * ck), [1.0]])
    for name, a in (("p1", p1), ("p2", p2), ("p3", p3)):
        p[name + "-lo"], p[name + "-hi"] = a < P_LO, a > P_HI
    p1c, p2c, p3c = (np.clip(a, P_LO, P_HI) for a in (p1, p2, p3))
    cum = np.concatenate([[1.0], np.cumprod(p2c[1:-1])])  # prod_{0 < l < k} p2[l], k = 1 .. M-1
    A0k = p1c[0] * cum * p3c[1:]
    Aii = p1c[:-1] * p3c[1:]
    uu = theta * e
    emis0, emis1, pi = np.exp(-uu), -np.expm1(-uu), pn.p_coal(t, c)
    for name, a in (("b", b), ("d", d), ("pi", pi), ("emis0", emis0), ("emis1", emis1), ("A0k", A0k), ("Aii", Aii)):
        p[name + "-lo"] = a < LO
        p[name + "-over"] = a > 1.0  # (1 - 1e-20 is 1.0 in float64: the upper clip acts on roundings above 1 only)
    return p


def tags_of(preds):
    return {name for name in BRANCH_TAGS if preds[name].any()}


def _same(p, q):
    return all(np.array_equal(p[k], q[k]) for k in p)


def stable(x, pat, theta, preds=None):
    """the first half of the admission rule: no predicate of this particle changes under +-1e-6 on any coordinate"""
    if preds is None:
        preds = branch_state(x, pat, theta)
    for i in range(len(x)):
        for s in (-PERTURB, PERTURB):
            y = np.array(x)
            y[i] += s
            if not _same(preds, branch_state(y, pat, theta)):
                return False
    return True


def numpy_block(x, pat, theta):
    return pn.from_dm(pn.particle_to_dm(x, pat, theta)).stack()


def torch_block(x, pat, theta):
    import torch

    from oracle import psmc_torch as pt

    with torch.no_grad():
        return pt.particle_to_params(torch.tensor(np.asarray(x, float)), pat, theta).numpy()


class MapCase(types.SimpleNamespace):
    def describe(self):
        reg = ",".join(f"{b}:{r}" for b, r in sorted(self.regimes.items())) or "-"
        return (f"seed={self.seed}.{self.sub} {self.kind} K={self.K} pat={self.pat} theta={self.theta:g} B={self.B} regimes[{reg}] "
                f"tags={'+'.join(sorted(self.tags))} oracles {self.oracles:.2e}")

    def label(self, b):
        return self.regimes.get(b, "wide" if self.kind == "wide" else "ordinary")


def _epoch_for(rng, where, P):
    if where == "first":
        return 0
    if where == "last":
        return P - 1
    if where == "mid":
        return int(rng.integers(1, P - 1)) if P > 2 else 0
    return int(rng.integers(0, P - 1))  # "any": not the last


def _apply(rng, x, single, P):
    name, where, val = single
    if where == "t1":
        x[0] = val
    elif where == "tM":
        x[1] = val
    elif where == "rho":
        x[2 + P] = val
    else:
        x[2 + _epoch_for(rng, where, P)] = val


def _candidate(seed, sub):
    rng = np.random.default_rng([41_000, seed, sub])
    idx = seed % 10
    K = K_CYCLE[idx]
    j = seed // 10
    c = MapCase(seed=seed, sub=sub, K=K, pat=PATTERNS[K], kind="wide" if (j + idx) % 2 else "regime", regimes={})
    # (K = 64 at theta = 1e-2 only: at 1e-4 the b row, ~ rho t_M ~ 1e-4, stands on 126 accumulated 3 x 3 products of entries of size 1
    # and ordinary particles part the oracles by 1.3e-11, just over the admission bar)
    c.theta = theta = 1e-2 if K == 64 else THETAS[(j // 2 + idx // 2) % 2]
    P = c.P = len(pn.parse_pattern(c.pat))
    # (the autograd reference of the Jacobian is the slow part of a case: 5 s per particle at K = 64, 1 s at K = 32)
    c.B = B = int(rng.integers(3, {64: 4, 32: 7}.get(K, 10)))
    x0 = pn.particle_from_linear(c.pat, 1e-4, 15.0, np.ones(P), theta, 2.0 * theta)
    if c.kind == "wide":  # a sigma = 4 population (variance, as mcmc.py:186-195 counts it)
        # at theta = 1e-2 only: with theta = 1e-4 the largest b_j is ~ rho t_M ~ 1e-5 while every b_j is a difference of two numbers
        # of size 1, the two oracles part by more than 1e-11 on a third of such populations, and the rejection cap would not hold
        c.theta = 1e-2
        c.B = B = int(rng.integers(3, 4 if K == 64 else (5 if K >= 16 else 7)))
        c.X = x0[None] + 2.0 * rng.normal(size=(B, P + 3))
        return c
    c.X = X = x0[None] + 0.5 * rng.normal(size=(B, P + 3))  # N(0, 0.25)
    n = 3 * seed  # running number of the regime slots: every single comes up in turn, every third slot is a pair
    for slot, b in enumerate(sorted(rng.choice(B, size=int(rng.integers(1, 4)), replace=False).tolist())):
        i = n + 5 * slot
        first = SINGLES[i % len(SINGLES)]
        name = first[0]
        _apply(rng, X[b], first, P)
        if i % 3 == 2:
            second = SINGLES[int(rng.integers(len(SINGLES)))]
            # (not tM6 with rho+-40: at rho = 10 theta and t_M = 400 the last d_k is 1 - 1 = a rounding residue against the 1e-20 clip,
            # at rho = 0.1 theta the b row is ~1e-4 of its rounding unit; the oracles part on most such pairs)
            if second[1] != first[1] and {first[1], second[1]} != {"tM", "rho"}:
                _apply(rng, X[b], second, P)
                name += "+" + second[0]
        c.regimes[b] = name
    return c


def _admit(c):
    """-> reason for rejection, or None; fills in the oracles' blocks, their distance and the tags"""
    preds = []
    for b in range(c.B):
        preds.append(branch_state(c.X[b], c.pat, c.theta))
    c.want = np.stack([numpy_block(xb, c.pat, c.theta) for xb in c.X])
    c.want_torch = np.stack([torch_block(xb, c.pat, c.theta) for xb in c.X])
    if not (np.isfinite(c.want).all() and np.isfinite(c.want_torch).all()):
        return "an oracle is not finite"
    c.oracles_by_particle = [row_scaled(c.want_torch[b], c.want[b]) for b in range(c.B)]
    c.oracles = max(c.oracles_by_particle)
    if c.oracles > ORACLES_AGREE:
        return f"the oracles part by {c.oracles:.2e}"
    # the rows the 1e-20 clip acts on directly; entries at it in one oracle must be at it in the other
    clipped = [0, 1, 4, 5, 6]
    if not np.array_equal(c.want[:, clipped] == LO, c.want_torch[:, clipped] == LO):
        return "the oracles clip different entries"
    for b in range(c.B):
        if not stable(c.X[b], c.pat, c.theta, preds[b]):
            return f"particle {b}: a branch predicate changes under +-{PERTURB:g}"
    c.preds = preds
    c.tags_by_particle = [tags_of(p) for p in preds]
    c.tags = set().union(*c.tags_by_particle)
    return None


@functools.lru_cache(maxsize=None)
def draw_map(seed):
    """Deterministic, CPU only -> the admitted case; ``case.rejected`` lists (sub-seed, reason) of the candidates before it."""
    rejected = []
    for sub in range(20):
        c = _candidate(int(seed), sub)
        why = _admit(c)
        if why is None:
            c.rejected = rejected
            return c
        rejected.append((sub, why))
    raise RuntimeError(f"seed {seed}: twenty candidates rejected: {rejected}")


def clip_mask(want):
    """[..., 7, K] bool: the entries of rows b, d, emis0, emis1, pi that the oracle has at the 1e-20 clip (the structural zeros
    b[K-1] = 0 are not among them)"""
    m = np.zeros(want.shape, dtype=bool)
    for r in (0, 1, 4, 5, 6):
        m[..., r, :] = want[..., r, :] == LO
    return m


def mp_block(x, pat, theta):
    """The map in 60-digit arithmetic (mpmath) -> [7][K] of mpf, clips included; ``x`` a list of mpf.  It follows the same branches
    as the oracle (an admitted particle is far from every threshold) and exists to measure the error of the float64 references
    themselves: where c dt is in the hundreds, exp(u - v) of transition.py:9-34 loses three digits in every float64 evaluation."""
    import mpmath as mp

    epochs = pn.parse_pattern(pat)
    P, M = len(epochs), sum(epochs)
    lo, plo, phi = mp.mpf("1e-20"), mp.mpf("1e-8"), 1 - mp.mpf("1e-8")
    clip = lambda v, a, b: a if v < a else (b if v > b else v)  # noqa: E731
    one = mp.mpf(1)  # (1 - 1e-20 is 1.0 in float64)
    t1 = mp.exp(x[0])
    tM = t1 + mp.exp(x[1])
    t = [mp.mpf(0)] + [mp.exp(mp.log(t1) + (mp.log(tM) - mp.log(t1)) * mp.mpf(k) / (M - 2)) for k in range(M - 1)]
    c = [mp.log(1 + mp.exp(v)) for v, w in zip(x[2:2 + P], epochs) for _ in range(w)]
    rho = (mp.mpf("0.1") + mp.mpf("9.9") / (1 + mp.exp(-x[2 + P]))) * theta
    e = []
    for k in range(M - 1):
        dt = t[k + 1] - t[k]
        if abs(c[k]) <= 1e-8:
            e.append((t[k] + t[k + 1]) / 2)
        elif c[k] > 100:
            e.append(t[k])
        else:
            e.append(1 / c[k] + t[k] - dt / mp.expm1(c[k] * dt))
    e.append(t[M - 1] + 1 / c[M - 1])
    e = [max(v, lo) for v in e]

    def expQ(r, cc):
        u, v, w = mp.sqrt(4 * cc * cc + r * r) / 2, (r + 2 * cc) / 2, (r - 2 * cc) / 2
        T1 = (mp.exp(u - v) + mp.exp(-(u + v))) / 2
        T2 = mp.exp(-v) * (1 + one / 6) if u < 1e-6 else (mp.exp(u - v) - mp.exp(-(u + v))) / 2 / u
        P11, P12, P21, P22 = T1 - w * T2, r * T2, cc * T2, T1 + w * T2
        return [[P11, P12, 1 - P11 - P12], [P21, P22, 1 - P21 - P22], [0, 0, 1]]

    taug = [v for pair in zip(t, e) for v in pair]
    row = [one, mp.mpf(0), mp.mpf(0)]
    rows = [row]
    for k in range(2 * M - 1):
        dtk = taug[k + 1] - taug[k]
        if abs(dtk) > 1e-8:
            Pm = expQ(2 * dtk * rho, dtk * c[k // 2])
            row = [sum(row[i] * Pm[i][j] for i in range(3)) for j in range(3)]
        rows.append(row)
    Rt, Re = rows[0::2], rows[1::2]
    b = [clip(Rt[j + 1][2] - Rt[j][2], lo, one) for j in range(M - 1)] + [mp.mpf(0)]
    d, p1, p2, p3 = [], [], [], []
    for j in range(M):
        last = j == M - 1
        gap = mp.mpf(0) if last else (t[j + 1] - e[j]) * c[j]
        d.append(clip(Re[j][0] + Re[j][1] * (one if last else -mp.expm1(-gap)) + Re[j][2] - Rt[j][2], lo, one))
        p1.append(clip(Re[j][1] * (0 if last else mp.exp(-gap)), plo, phi))
        p2.append(clip(mp.mpf(0) if last else mp.exp(-(t[j + 1] - t[j]) * c[j]), plo, phi))
        p3.append(clip(one if last else -mp.expm1(-(t[j + 1] - t[j]) * c[j]), plo, phi))
    u, v, cum, A01 = [mp.mpf(0)] * M, [mp.mpf(0)] * M, one, None
    for k in range(1, M):
        A0k = clip(p1[0] * cum * p3[k], lo, one)
        A01 = A0k if k == 1 else A01
        v[k] = A0k / A01
        u[k - 1] = clip(p1[k - 1] * p3[k], lo, one) / v[k]
        cum = cum * p2[k]
    emis0 = [clip(mp.exp(-theta * ek), lo, one) for ek in e]
    emis1 = [clip(-mp.expm1(-theta * ek), lo, one) for ek in e]
    H, S = mp.mpf(0), []
    for k in range(M - 1):
        H += c[k] * (t[k + 1] - t[k])
        S.append(mp.exp(-H))
    S.append(mp.mpf(0))
    Ci = [S[k] - S[k + 1] for k in range(M - 1)]
    pi = [clip(1 - sum(Ci), lo, one)] + [clip(v_, lo, one) for v_ in Ci]
    return [b, d, u, v, emis0, emis1, pi]


def mp_values_and_jvp(x, pat, theta, tan=None):
    """-> ([7, K] values, [7, K] J tan or None) as float64, from ``mp_block``; the JVP by a central difference with step 1e-25"""
    import mpmath as mp

    with mp.workdps(60):
        x = [mp.mpf(float(a)) for a in x]
        val = np.array([[float(v) for v in r] for r in mp_block(x, pat, theta)])
        if tan is None:
            return val, None
        h = mp.mpf("1e-25")
        up = mp_block([a + h * mp.mpf(float(s)) for a, s in zip(x, tan)], pat, theta)
        dn = mp_block([a - h * mp.mpf(float(s)) for a, s in zip(x, tan)], pat, theta)
        return val, np.array([[float((p - m) / (2 * h)) for p, m in zip(ru, rd)] for ru, rd in zip(up, dn)])


def log_prior_torch(x, P, alpha, beta):
    """model.py:11-21 restated in torch for autograd: logN(log(rho / theta); 0, 1) - alpha sum diff(log c)^2 - beta |x|^2"""
    import torch

    z = torch.log(0.1 + 9.9 * torch.sigmoid(x[2 + P]))
    log_c = torch.log(torch.logaddexp(x[2:2 + P], torch.zeros_like(x[2:2 + P])))  # jax.nn.softplus: no threshold
    return -0.5 * z * z - 0.5 * math.log(2.0 * math.pi) - alpha * (torch.diff(log_c) ** 2).sum() - beta * (x * x).sum()


# ------------------------------------------------------------------------------------------------- part B: the update
LD = np.longdouble
U = 2.0 ** -53  # unit roundoff of float64
TINY = float(np.finfo(np.float64).smallest_subnormal)
DS = (1, 2, 17, 63, 64, 65, 67, 72)  # 256 / D = 256 ... 3 parts of the workgroup, with and without idle lanes
BS = (1, 2, 3, 15, 16, 17, 255, 256, 257)  # around the 16-particle tile of the distances and the 256-thread stride of the kernel row
B1, B2, EPS = 0.9, 0.999, 1e-8


def pairwise(x):
    """the B (B - 1) / 2 distances of the strict lower triangle, row-major (pair (i, j), i > j, at i (i - 1) / 2 + j), longdouble"""
    x = np.asarray(x, dtype=LD)
    out = [np.sqrt(((x[i] - x[:i]) ** 2).sum(1)) for i in range(1, x.shape[0])]
    return np.concatenate(out) if out else np.zeros(0, dtype=LD)


def median_heuristic(x):
    """median(pairwise distances)^2 / log B (1 for a single particle), longdouble"""
    d = np.sort(pairwise(x))
    if d.size == 0:
        return LD(1.0)
    m = d.size
    med = d[m // 2] if m % 2 else (d[m // 2 - 1] + d[m // 2]) / LD(2)
    return med * med / np.log(LD(x.shape[0]))


def svgd_reference(x, g, mu, nu, nu_max, h, count, lr, b1=B1, b2=B2, eps=EPS):
    """One step in longdouble, one column j at a time (vectorised over i and the coordinates) -> dict with mu, nu, nu_max, x_out
    and ``bound_*``: forward-error bounds of a float64 evaluation in any order of summation, from absolute sums.

    phi_j = (1/B) sum_i k_ij (2/h (x_i - x_j) - g_i).  With a_j = (1/B) sum_i k_ij (|2/h (x_i - x_j)| + |g_i|) a float64
    evaluation errs by at most gamma a_j, gamma = (B + 2 D + 16) 2^-53 (B additions, the products, the division, exp's own
    rounding and 2 / h), plus what the rounding of the exponent does to k_ij: d2 carries D + 1 roundings and the division one,
    so k_ij is off by the factor exp(+-(d2_ij / h) (D + 3) 2^-53).  The state's own terms (b1 mu, the final addition) add one
    rounding each; this is stated here because the state is not zero.  nu, nu_max and x_out follow by the same first-order
    propagation (phi^2, the division by the bias correction, the square root, the quotient)."""
    x, g, mu0, nu0, nm0 = (np.asarray(a, dtype=LD) for a in (x, g, mu, nu, nu_max))
    h, b1, b2, eps, lr = LD(h), LD(b1), LD(b2), LD(eps), LD(lr)
    B, D = x.shape
    phi, a_sum, e_sum = (np.zeros((B, D), dtype=LD) for _ in range(3))
    two_over_h = LD(2) / h
    for j in range(B):
        diff = x - x[j]
        d2 = (diff * diff).sum(1)
        k = np.exp(-d2 / h)[:, None]
        phi[j] = (k * (two_over_h * diff - g)).sum(0) / B
        mag = np.abs(two_over_h * diff) + np.abs(g)
        a_sum[j] = (k * mag).sum(0) / B
        # (an off-diagonal kernel value that float64 flushes to a subnormal or to 0 is off by up to the smallest subnormal)
        e_sum[j] = ((k * (d2 / h)[:, None] * (D + 3) * U + TINY) * mag).sum(0) / B
    gamma = (B + 2 * D + 16) * U
    e_phi = gamma * a_sum + e_sum
    one = LD(1)
    mu = b1 * mu0 + (one - b1) * phi
    e_mu = (one - b1) * e_phi + U * (np.abs(b1 * mu0) + np.abs(mu))
    nu = b2 * nu0 + (one - b2) * phi * phi
    e_nu = (one - b2) * (2 * np.abs(phi) * e_phi + e_phi * e_phi + 3 * U * phi * phi) + U * (np.abs(b2 * nu0) + np.abs(nu))
    den1, den2 = one - b1 ** int(count), one - b2 ** int(count)
    # the bias corrections 1 - b^count are float64 on the host: the power's rounding, 2^-53 b^count, is left standing against the
    # difference -- 500 roundings of 1 - 0.999^2.  (Plain float64 numpy missed the bound without this term by a factor 18.)
    r1, r2 = (2 * U * b ** int(count) / den + 2 * U for b, den in ((b1, den1), (b2, den2)))
    nu_hat = nu / den2
    e_nm = e_nu / den2 + (r2 + 2 * U) * np.abs(nu_hat)
    nm = np.maximum(nm0, nu_hat)  # (max is 1-Lipschitz)
    root = np.sqrt(nm)
    root_lo = np.sqrt(np.maximum(nm - e_nm, 0))
    e_s = (root - root_lo) + U * (root + eps)
    s = root + eps
    mu_hat = mu / den1
    upd = lr * mu_hat / s
    e_upd = np.abs(lr) * ((e_mu / den1 + (r1 + 2 * U) * np.abs(mu_hat)) / s + np.abs(mu_hat) * e_s / (s * np.maximum(s - e_s, eps / 2))) + 3 * U * np.abs(upd)
    x_out = x - upd
    e_x = e_upd + U * np.abs(x_out)
    return {"phi": phi, "mu": mu, "nu": nu, "nu_max": nm, "x_out": x_out, "bound_mu": e_mu + TINY, "bound_nu": e_nu + TINY,
            "bound_nu_max": e_nm + TINY, "bound_x_out": e_x + TINY, "gamma": gamma}


def svgd_float64(x, g, mu, nu, nu_max, h, count, lr, b1=B1, b2=B2, eps=EPS):
    """the same formulas in plain float64 numpy: the evidence a bound of ``svgd_reference`` is judged by, should correct code
    seem to miss it"""
    x, g = np.asarray(x, float), np.asarray(g, float)
    B, D = x.shape
    phi = np.zeros((B, D))
    for j in range(B):
        diff = x - x[j]
        k = np.exp(-(diff * diff).sum(1) / h)[:, None]
        phi[j] = (k * ((2.0 / h) * diff - g)).sum(0) / B
    m = b1 * mu + (1.0 - b1) * phi
    v = b2 * nu + (1.0 - b2) * phi * phi
    nm = np.maximum(nu_max, v / (1.0 - b2 ** count))
    return {"mu": m, "nu": v, "nu_max": nm, "x_out": x - lr * (m / (1.0 - b1 ** count)) / (np.sqrt(nm) + eps)}


class UpdateCase(types.SimpleNamespace):
    def describe(self):
        return (f"seed={self.seed} B={self.B} D={self.D} count={self.count} lr={self.lr:g} h_in={self.h_factor:g} x median heuristic"
                f"{' twins' if self.twins else ''}")

    def reference(self):
        if getattr(self, "_ref", None) is None:
            self._ref = svgd_reference(self.x, self.g, self.mu, self.nu, self.nu_max, self.h_in, self.count, self.lr)
        return self._ref


@functools.lru_cache(maxsize=None)
def draw_update(seed):
    seed = int(seed)
    rng = np.random.default_rng([42_000, seed])
    c = UpdateCase(seed=seed)
    c.D = D = DS[seed % 8]
    c.B = B = BS[(seed // 8 + 2 * (seed % 8)) % 9]
    c.x = rng.normal(size=(B, D))
    c.twins = bool(B >= 3 and rng.integers(3) == 0)  # (two identical particles alone have the median distance 0)
    if c.twins:
        i, j = rng.choice(B, size=2, replace=False)
        c.x[i] = c.x[j]
    c.g = rng.normal(size=(B, D)) * float(rng.choice([0.1, 1.0, 30.0]))
    # a running AMSGrad state: non-zero moments, nu_max at or above some nu
    c.mu = rng.normal(size=(B, D)) * 0.3
    c.nu = rng.normal(size=(B, D)) ** 2 * 0.1
    c.nu_max = np.where(rng.random((B, D)) < 0.5, c.nu * rng.uniform(1.0, 3.0, size=(B, D)), c.nu * rng.uniform(0.0, 1.0, size=(B, D)))
    c.count = int(rng.choice([1, 2, 1000]))
    c.lr = float(rng.choice([0.0, 0.1]))
    c.h_factor = float(rng.choice([1e-3, 1.0, 1e4]))  # at 1e-3 every off-diagonal kernel value underflows to 0 (D > 2)
    c.h_in = float(median_heuristic(c.x)) * c.h_factor if B > 1 else c.h_factor
    return c


# ------------------------------------------------------------------------------------------------- part B: the select
def _cluster_sizes(B, target):
    """sizes (largest first, each >= 2) of tight clusters among B particles, the rest far from everything, such that exactly
    ``target`` pairs lie within a cluster"""
    tri = lambda m: m * (m - 1) // 2  # noqa: E731

    def rec(left, need, cap):
        if need == 0:
            return []
        for m in range(min(cap, left), 1, -1):
            if tri(m) <= need:
                rest = rec(left - m, need - tri(m), m)
                if rest is not None:
                    return [m] + rest
        return None

    sizes = rec(B, target, B)
    assert sizes is not None, (B, target)
    return sizes


SELECT_CASES = (
    [("outlier", B, D) for B in (120, 300, 600) for D in (1, 18)]
    + [("clusters", B, D) for B in (40, 42, 300, 302) for D in (1, 18)]  # 780 / 44,850 distances: even; 861 / 45,451: odd
    + [("line", B, D) for B in (100, 300) for D in (1, 18)]
    + [("denormal", B, 1) for B in (3, 4)]
    + [("normal", B, D) for B in (257, 258) for D in (1, 18)]  # 32,896 (even) and 33,153 (odd): the first sizes of the chip-wide select
)


@functools.lru_cache(maxsize=None)
def select_population(kind, B, D):
    """[B, D] float64.
    outlier   one particle 1e6 away from a normal cloud: all but B - 1 distances fall into bucket 0 of 2,048 -- at 120 particles
              7,021 of 7,140 (more than the 4,096 the select gathers: the narrowing path, thousands of distinct values), beyond
              256 particles a candidate list of nearly all n in the chip-wide select.
    clusters  tight clusters (and singletons) 40 apart, sizes chosen so that exactly floor((n - 1) / 2) + 1 distances lie
              within a cluster: the lower middle rank is the largest of them and, for an even n, the upper middle rank the
              smallest distance between clusters -- the two ranks in different buckets, `below` > 0 in the chip-wide select.
    line      x_i = a + i ulp(a) in every coordinate: distances that differ by single ulps, many of them equal.
    denormal  D = 1, x = (0, 0, 1.8e-162[, 1e-150]): the distances are 0, and sqrt(fl(3.24e-324)) = sqrt(2^-1074) = 2.2e-162
              twice -- the square is the smallest subnormal.  With B = 3 the range of the select is [0, 2.2e-162] and its
              `scale` = 2047 / 2.2e-162 = 9.2e164, finite: bucket 0 and bucket 2047.  (A distance is a square root: it is 0 or at
              least 2.2e-162, never subnormal itself.)
    normal    a standard normal cloud."""
    rng = np.random.default_rng([43_000, B, D, len(kind)])
    if kind == "outlier":
        x = rng.normal(size=(B, D))
        x[int(rng.integers(B))] += 1e6 / math.sqrt(D)
    elif kind == "clusters":
        n = B * (B - 1) // 2
        sizes = _cluster_sizes(B, (n - 1) // 2 + 1)
        groups = sizes + [1] * (B - sum(sizes))
        centre = np.repeat(np.arange(len(groups), dtype=np.float64) * 40.0, groups)
        x = 0.3 * rng.normal(size=(B, D))
        x[:, 0] += centre
        x = x[rng.permutation(B)]
    elif kind == "line":
        a = rng.uniform(1.0, 2.0, size=D)
        x = a[None] + np.arange(B)[:, None] * np.spacing(a)[None]
    elif kind == "denormal":
        x = np.array([0.0, 0.0, 1.8e-162, 1e-150][:B])[:, None]
    else:
        x = rng.normal(size=(B, D))
    return np.ascontiguousarray(x, dtype=np.float64)
