"""Models with massless states (tests/massless_fuzz.py: pi = b = v = 0 on a set of dead states) through the likelihood and gradient
kernels, posterior decoding and Viterbi, each against its float64 oracle.

CPU: the conditions a valid draw meets on the reference alone, for every default seed and forced case; the coverage of the default
seeds; the comparators against the oracle's own output with one fault injected.  GPU: ``_run_case`` of tests/test_model_fuzz.py on
the new draws (its bars, its contract: a call whose underflow flag stays clear is accurate, one that raises it is accurate once
repeated at rescale interval 1); ``compare_posterior`` / ``compare_viterbi`` of tests/decode_fuzz.py plus what only these models can
show -- posterior mass of exactly 0 on every dead state, no path through a dead state, the oracle's path where it is the only one;
and the ordinary neighbours of a particle whose gradient float32 cannot hold (``massless_fuzz.NEIGHBOUR_CASES``).
``pytest -s -m gpu tests/test_massless_fuzz.py`` prints one line per draw; with PHK_MASSLESS_FUZZ_REPORT=<file> the summary of the
run is written there (profiles/massless_fuzz.txt).
"""

from __future__ import annotations

import collections
import os
import warnings

import numpy as np
import pytest

import decode_fuzz as df
import massless_fuzz as mm
import model_fuzz as mf
import test_decode_fuzz as tdf
import test_model_fuzz as tmf
from parity_bars import F32_GRAD_FULL, F32_GRAD_OWN, grad_error_ratios

DEFAULT_SEEDS = 80
DECODE_SEEDS = 40
N_SEEDS = int(os.environ.get("PHK_MASSLESS_FUZZ_SEEDS", str(DEFAULT_SEEDS)))
N_DECODE = int(os.environ.get("PHK_MASSLESS_FUZZ_DECODE_SEEDS", str(DECODE_SEEDS)))
MIN_PER_TAG = 4
WANTED_TAGS = tuple(f"pat:{p}" for p in mm.PATTERNS) + ("pat:per-chunk", "family:dense16", "family:lanes", "plan:variant", "plan:serial",
                                                        "plan:segmented", "plan:hybrid", "plan:tuner", "f32", "f64", "dlog", "f32-block",
                                                        "per-chunk", "beside-ordinary") + mm.FORMS
WAVE = 32  # sequences of a wave of the two-lane sweeps: the neighbourhood a wave-wide decision reaches
# cases that found something, kept by name: name -> forced case of massless_fuzz
REGRESSIONS = {
    # A particle whose only live state is the last one has a gradient of 1e98 ... 1e138 after 1,040 sites: float32 returns inf for it.
    # The exclusive scans of the two- and eight-lane layouts read a lane of the NEIGHBOURING sequence at a group's edge and
    # multiplied it by a 0 / 1 mask: inf * 0 = NaN, and every sequence of the 16-lane row came back NaN -- ll of the gradient call
    # and all seven gradient rows of ordinary particles, under the serial plan with the underflow flag clear.  The mask is now a bit
    # mask (Group in psmc_kernels.hip, the carry of scripts/gen_sweep_asm.py).
    "nan_in_the_neighbours_segmented": "top_live_segmented_3x2_1040",
    "nan_in_the_neighbours_serial_flag_clear": "top_live_serial_3x2_1040",
    "nan_in_the_neighbours_hybrid": "top_live_hybrid_3x2_1040",
    "nan_in_the_neighbours_two_waves": "top_live_segmented_33x2_2600",
    "nan_in_the_neighbours_eight_lanes": "top_live_lanes8_5x2_1040",
}


def _defaults():
    return [mm.draw(seed) for seed in range(DEFAULT_SEEDS)]


def _forced():
    return [mm.forced(name) for name in sorted(mm.FORCED)]


# ------------------------------------------------------------------------------------------------- CPU: the reference alone
def test_reference_alone_conditions():
    """100 % of the default seeds and of the forced cases, none redrawn: finite ll and gradient (W = 0 included), the float32 cap,
    every emis0 >= 0.5 (so that the raw gradient form of ``_run_case`` covers every particle, dead entries included)."""
    worst32 = 0.0
    for d in _defaults() + _forced():
        assert mm.oracle_conditions(d) == [], d.describe()
        assert d.odd and d.dead[d.odd].any() and not d.dead.all(-1).any(), d.describe()
        assert (d.P[..., mm.DEAD_ROWS, :][np.broadcast_to(d.dead[:, :, None, :], d.P[..., mm.DEAD_ROWS, :].shape)] == 0).all()
        assert (d.P[:, :, 1][d.dead] > 0).all() and (d.P[:, :, 4][d.dead] > 0).all()  # (d, u, emis0, emis1 stay as they were)
        if not d.dbl:
            worst32 = max(worst32, float(np.abs(mf.oracle(d)["g"]).max()))
        # the one-sided derivatives at the dead entries are not zero: a kernel that skipped dead states would be wrong there
        if not d.dlog:
            g = mf.oracle(d)["g"]
            dead = np.broadcast_to(d.dead[:, :1] if not d.per_chunk else d.dead, (d.B, d.S, d.K))
            # (row b or row v: with the lowest state alone alive nothing sits above a dead state, and its b entry is 0)
            assert max(np.abs(g[:, :, 0][dead]).max(), np.abs(g[:, :, 3][dead]).max()) > 0, d.describe()
    print(f"largest |d ll / d theta| of the oracle over the float32 draws: {worst32:.3e} (cap {mm.GRAD_CAP_F32:g})")
    # a single-live-state particle inside the cap at every K and at 513, 1040 and 2600 sites
    from oracle import cport

    for K in (4, 8, 16, 32, 64):
        for L in (513, 1040, 2600):
            rng = np.random.default_rng([43_000, K, L])
            P = mm.kill(mf.ordinary(rng, K), mm.dead_mask("one-mid", K, True))[None, None]
            ll, g = cport.batch(P, mm._rows(rng, 1, L, 0), np.array([0]), 0)
            assert np.isfinite(ll).all() and np.abs(g).max() <= mm.GRAD_CAP_F32, (K, L, float(np.abs(g).max()))


def test_decoder_references():
    """posterior: finite gamma, ll and emulation figure on every draw; at most a quarter of the float32 draws is run as float64
    (the project's rule, F32_REDRAW_BAR / 5 on the float32 emulation).  Viterbi: finite logp, a path that never visits a dead state;
    margins of +inf occur (no second path exists: the exact path is demanded)."""
    post = [mm.decode_draw(seed, "posterior") for seed in range(DECODE_SEEDS)]
    f32_default = [d for d in post if not (d.seed // 10) % 2]
    redrawn = [d.massless_seed for d in f32_default if d.redrawn]
    for d in post:
        o = df.oracle_posterior(d)
        assert np.isfinite(o["ll"]).all() and np.isfinite(o["E"]).all(), d.describe()
        for b in range(d.B):
            for s in range(d.S):
                g = o["gamma"][b][s]
                assert np.isfinite(g).all() and (g[:, mm.dead_of(d, b, s)] == 0).all(), d.describe()
    print(f"posterior: {len(redrawn)} of {len(f32_default)} float32 draws run as float64 (seeds {redrawn})")
    assert len(redrawn) <= 0.25 * len(f32_default)
    n_inf = 0
    for d in (mm.decode_draw(seed, "viterbi") for seed in range(DECODE_SEEDS)):
        o = df.oracle_viterbi(d)
        assert np.isfinite(o["logp"]).all(), d.describe()
        n_inf += int(np.isinf(o["margin"]).sum())
        for b in range(d.B):
            for s in range(d.S):
                assert not mm.dead_of(d, b, s)[o["path"][b][s].astype(int)].any(), d.describe()
    print(f"viterbi: {n_inf} sequences with a margin of +inf")
    assert n_inf >= 4


def test_default_seeds_cover_the_list():
    n = collections.Counter()
    for d in _defaults():
        n.update(d.tags)
    print(sorted(n.items()))
    for tag in WANTED_TAGS:
        assert n[tag] >= MIN_PER_TAG, (tag, n[tag])
    for L in mm.LS:
        assert sum(1 for d in _defaults() if d.L == L) >= MIN_PER_TAG
    for K in set(mf.KS):
        assert sum(1 for d in _defaults() if d.K == K) >= MIN_PER_TAG
    assert sum(1 for d in _defaults() if d.B == 33) >= MIN_PER_TAG and sum(1 for d in _defaults() if d.B == 40) >= MIN_PER_TAG
    for kind in ("posterior", "viterbi"):
        pats = collections.Counter()
        for seed in range(DECODE_SEEDS):
            d = mm.decode_draw(seed, kind)
            pats.update(set(d.patterns.values()))
            assert d.dead.any() and not d.dead.all(-1).any()
        for p in mm.PATTERNS:
            assert pats[p] >= MIN_PER_TAG, (kind, p, pats[p])
    assert mm.draw(3) is mm.draw(3) and np.array_equal(mm._draw(3).P, mm.draw(3).P)  # deterministic


# ------------------------------------------------------------------------------------------------- the comparators
def judge(d, ll, g, ll0):
    """the assertions of ``test_model_fuzz._run_case`` on one candidate (ll [B, S], g [B, S, 7, K], the no-gradient call's ll0)
    -> list of failures"""
    o = mf.oracle(d)
    out = []
    if not np.isfinite(g).all():
        out.append("gradient not finite")
    if not tmf._ll_ratio(ll, o["ll"], d.dbl, d.L, uncorrected=d.f32_block) <= 1.0:
        out.append("ll")
    if not tmf._nograd_ratio(ll0, ll, d.dbl, d.L) <= 1.0:
        out.append("no-gradient call")
    with np.errstate(invalid="ignore"):
        r_dlog, _, r_ord = tmf._grad_ratios(d, g, d.dbl)
    if not r_dlog < 1.0:
        out.append("theta * d ll / d theta")
    if r_ord == r_ord and not r_ord < 1.0:
        out.append("d ll / d theta, particle by particle")
    return out


def dead_mass(d, marginals):
    """largest posterior mass a call put on a dead state (must be exactly 0)"""
    worst = 0.0
    for b in range(d.B):
        for s in range(d.S):
            dead = mm.dead_of(d, b, s)
            if dead.any() and marginals[b, s].size:
                worst = max(worst, float(np.abs(marginals[b, s][:, dead]).max()))
    return worst


def dead_visits(d, path):
    """sites at which a Viterbi path [B, S, L - W] (255 past a row's own length) sits in a dead state"""
    n = 0
    for b in range(d.B):
        for s in range(d.S):
            z = path[b, s, : d.row_len(s) - d.W].astype(int)
            n += int(mm.dead_of(d, b, s)[np.minimum(z, d.K - 1)].sum())
    return n


def path_mismatch_where_unique(d, o, path):
    """sequences whose oracle margin is +inf (no second path of positive probability) and whose path is not the oracle's"""
    return [(b, s) for b in range(d.B) for s in range(d.S)
            if np.isinf(o["margin"][b, s]) and not np.array_equal(path[b, s, : d.row_len(s) - d.W], o["path"][b][s])]


def test_comparators_catch_seeded_faults():
    """The oracle's own output passes; each fault, wrong numbers only, is rejected."""
    d = next(d for d in _defaults() if not d.dlog and not d.dbl and d.B >= 4 and len(d.odd) < d.B and d.L >= 513 and d.W == 0)
    o = mf.oracle(d)
    assert judge(d, o["ll"], o["g"], o["ll"]) == []
    # the gradient zeroed at the dead entries of b, v and pi: what a sweep that skipped dead states would return
    g = o["g"].copy()
    dead = np.broadcast_to(d.dead if d.per_chunk else d.dead[:, :1], (d.B, d.S, d.K))
    for r in mm.DEAD_ROWS:
        g[:, :, r][dead] = 0.0
    assert "d ll / d theta, particle by particle" in judge(d, o["ll"], g, o["ll"])
    # one particle NaN (ll, then its gradient), then the whole wave-sized neighbourhood
    b = d.odd[0]
    ll = o["ll"].copy()
    ll[b] = np.nan
    assert "ll" in judge(d, ll, o["g"], o["ll"])
    g = o["g"].copy()
    g[b] = np.nan
    assert "gradient not finite" in judge(d, o["ll"], g, o["ll"])
    ll, g = o["ll"].copy(), o["g"].copy()
    ll[max(0, b - WAVE): b + WAVE] = np.nan
    g[max(0, b - WAVE): b + WAVE] = np.nan
    bad = judge(d, ll, g, o["ll"])
    assert "ll" in bad and "gradient not finite" in bad and "theta * d ll / d theta" in bad
    # ll of a massless particle replaced by that of its parent, whose states all carry mass
    from oracle import cport

    ll = o["ll"].copy()
    ll[b] = cport.batch(d.P_parent[b:b + 1], d.data, d.inds, d.W)[0][0]
    assert "ll" in judge(d, ll, o["g"], o["ll"])

    # posterior: 1e-7 of every site's mass moved into a dead state, renormalised -- inside every bar of compare_posterior
    d = next(d for d in (mm.decode_draw(seed, "posterior") for seed in range(DECODE_SEEDS))
             if d.marginals and d.nbin and not d.dbl and d.dead[0, 0].any())
    o = df.oracle_posterior(d)
    good = df.posterior_candidate(d, o["gamma"], o["ll"])
    assert df.compare_posterior(o, good, d)[0] <= 1.0 and dead_mass(d, good["marginals"]) == 0.0
    G = [[g.copy() for g in row] for row in o["gamma"]]
    k = int(np.nonzero(mm.dead_of(d, 0, 0))[0][0])
    G[0][0][:, k] += 1e-7
    G[0][0] /= G[0][0].sum(-1, keepdims=True)
    bad = df.posterior_candidate(d, G, o["ll"])
    assert df.compare_posterior(o, bad, d)[0] <= 1.0  # (the bars alone would let it through)
    assert dead_mass(d, bad["marginals"]) > 0.0

    # Viterbi: one visit to a dead state
    d = next(d for d in (mm.decode_draw(seed, "viterbi") for seed in range(DECODE_SEEDS)) if d.L - d.W >= 30 and d.dead[0, 0].any())
    o = df.oracle_viterbi(d)
    good = df.viterbi_candidate(d, o["path"], o["logp"])
    assert df.compare_viterbi(o, good, d)[0] <= 1.0 and dead_visits(d, good["path"]) == 0
    assert path_mismatch_where_unique(d, o, good["path"]) == []
    bad = dict(good, path=good["path"].copy())
    bad["path"][0, 0, (d.row_len(0) - d.W) // 2] = int(np.nonzero(mm.dead_of(d, 0, 0))[0][0])
    assert dead_visits(d, bad["path"]) == 1 and df.compare_viterbi(o, bad, d)[0] > 1.0


# ------------------------------------------------------------------------------------------------- GPU
NEIGHBOURS: list[dict] = []
DECODE: list[dict] = []
_first_record = [None]


@pytest.fixture(scope="module", autouse=True)
def _report():
    _first_record[0] = len(tmf.RECORDS)
    yield
    path = os.environ.get("PHK_MASSLESS_FUZZ_REPORT")
    if path and (tmf.RECORDS[_first_record[0]:] or NEIGHBOURS or DECODE):
        with open(path, "w") as f:
            f.write(summary(tmf.RECORDS[_first_record[0]:], NEIGHBOURS, DECODE))


def summary(records, neighbours, decode):
    out = [f"massless-state fuzz: {len(records)} likelihood draws, {sum(1 for r in records if r['failures'])} over a bar\n",
           f"{'regime':<14}{'type':<5}{'draws':>6}{'ll err':>11}{'ll/bar':>9}{'nograd/bar':>11}{'kern/bar':>9}{'err/bound':>10}{'raw, by particle':>17}"
           f"{'flag':>6}{'flag@1':>7}\n"]
    for regime in mm.FORMS + ("forced",):
        for ft in ("f32", "f64"):
            rs = [r for r in records if r["regime"] == regime and r["ft"] == ft]
            if rs:
                mx = lambda k, rs=rs: max((r[k] for r in rs if r[k] == r[k]), default=float("nan"))  # noqa: E731
                out.append(f"{regime:<14}{ft:<5}{len(rs):>6}{mx('ll_err'):>11.2e}{mx('ll'):>9.3f}{mx('nograd'):>11.3f}{mx('kern'):>9.3f}"
                           f"{mx('grad'):>10.3f}{mx('raw_ord'):>17.3f}{sum(r['flag'] for r in rs):>6}{sum(r['flag1'] for r in rs):>7}\n")
    for r in records:
        if r["failures"]:
            out.append(f"OVER seed={r['seed']}: {'; '.join(r['failures'])}\n")
    for r in neighbours:
        out.append(f"neighbours of a particle beyond float32, {r['name']}: flag={r['flag']} flag@1={r['flag1']} ordinary particles: ll {r['ll']:.3f} x "
                   f"its bar, no-gradient call {r['nograd']:.3f}, d ll / d theta {r['raw']:.3f} x its bound; the particle itself: "
                   f"{r['own_nonfinite']} non-finite entries\n")
    for kind in ("posterior", "viterbi"):
        for ft in ("f32", "f64"):
            rs = [r for r in decode if r["kind"] == kind and r["ft"] == ft]
            if rs:
                w = max(rs, key=lambda r: r["ratio"])
                out.append(f"{kind} {ft}: {len(rs)} draws, worst error/bar {w['ratio']:.3f} (seed {w['seed']}), flag raised {sum(r['flag'] for r in rs)}, "
                           + (f"largest mass on a dead state {max(r['dead'] for r in rs):g}, {sum(r['redrawn'] for r in rs)} float32 draws run as float64\n"
                              if kind == "posterior" else
                              f"visits to a dead state {sum(r['dead'] for r in rs)}, sequences with a unique path {sum(r['unique'] for r in rs)}\n"))
    return "".join(out)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_likelihood_and_gradient(seed):
    """``_run_case`` of tests/test_model_fuzz.py: ll, the no-gradient call, theta * d ll / d theta, the raw d ll / d theta particle by
    particle (every particle of these draws: all emis0 >= 0.5), the plugin surface; flag clear -> accurate, flag raised -> accurate
    at interval 1; NaN or inf never."""
    tmf._run_case(mm.draw(seed))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(mm.FORCED))
def test_forced_cases(name):
    """the plan of the note in tests/test_sweep_valu.py and its serial and hybrid siblings, a one-live-state particle (and every
    other pattern) among ordinary ones"""
    tmf._run_case(mm.forced(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REGRESSIONS))
def test_regressions(name):
    """The ordinary neighbours of a particle whose gradient float32 cannot hold: ll, the no-gradient call and d ll / d theta of every
    ORDINARY particle to the bars of ``_run_case``, whatever the call returns for the particle itself (the oracle's own gradient
    of it is 1e98 and more; at 2,600 sites NaN)."""
    d = mm.forced(REGRESSIONS[name])
    o = mf.oracle(d)
    others = [b for b in range(d.B) if b not in d.odd]
    assert len(others) >= 2 and np.isfinite(o["ll"][others]).all() and np.isfinite(o["g"][others]).all()
    eng = tmf._engine(d)
    eng.set_rescale_interval(d.nrm)
    eng.set_autotune(False)
    tmf._apply_plan(eng, d.plan)
    ll, g, flag, ll0, flag0 = tmf._calls(eng, d, d.plan)
    rec = {"name": name, "flag": int(flag or flag0), "flag1": 0}
    if flag or flag0:
        eng.set_rescale_interval(1)
        ll, g, f1, ll0, f01 = tmf._calls(eng, d, d.plan)
        rec["flag1"] = int(f1 or f01)  # (the particle beyond float32 keeps the flag up: recorded, not asserted)
    rec["own_nonfinite"] = int((~np.isfinite(g[d.odd])).sum())
    assert np.isfinite(ll[others]).all() and np.isfinite(ll0).all() and np.isfinite(g[others]).all(), \
        f"non-finite results for ordinary particles {sorted({int(b) for b in np.argwhere(~np.isfinite(g))[:, 0]} - set(d.odd))}"
    rec["ll"] = tmf._ll_ratio(ll[others], o["ll"][others], d.dbl, d.L)
    rec["nograd"] = tmf._nograd_ratio(ll0[others], ll[others], d.dbl, d.L)
    rec["raw"] = max(grad_error_ratios(g[b:b + 1], o["g"][b:b + 1], None, d.P_model[b:b + 1], F32_GRAD_OWN, F32_GRAD_FULL)[0] for b in others)
    NEIGHBOURS.append(rec)
    print(f"massless neighbours {d.describe()}: {rec}")
    assert rec["ll"] <= 1.0 and rec["nograd"] <= 1.0 and rec["raw"] < 1.0, rec


def _decode_calls(d, eng, call):
    """a decode call; one that raises the underflow flag is repeated at rescale interval 1, where the flag must stay clear"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = call()
        flag = bool(eng.underflow_risk())
        if flag:
            assert d.nrm > 1, "underflow flag raised at interval 1"
            eng.set_rescale_interval(1)
            out = call()
            assert not eng.underflow_risk(), "underflow flag raised at interval 1"
    return out, flag


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_DECODE))
def test_posterior(seed):
    import torch

    d = mm.decode_draw(seed, "posterior")
    o = df.oracle_posterior(d)
    kern, eng, pp, P, inds = tdf._setup(d)
    forced = d.plan is not None
    if forced:
        eng.set_plan(1 if d.plan[0] == "segmented" else 0, *d.plan[1:])
    vals = None if d.values is None else torch.as_tensor(d.values, dtype=torch.float64).cuda()

    def call():
        if d.raw:
            return eng.posterior(P, inds, d.W, values=vals, bin=d.bin, marginals=d.marginals, mean=vals is not None)
        return kern.posterior(pp, d.inds, values=d.values, bin=d.bin, marginals=d.marginals)

    a, flag = _decode_calls(d, eng, call)
    cand = {"ll": a[0].cpu().numpy(), "mean": None if a[1] is None else a[1].double().cpu().numpy(),
            "marginals": None if a[2] is None else a[2].double().cpu().numpy()}
    ratio, msg, info = df.compare_posterior(o, cand, d)
    dead = dead_mass(d, cand["marginals"]) if cand["marginals"] is not None else 0.0
    print(f"massless posterior {d.describe()}: nbin={d.nbin} flag={int(flag)} max |gamma - oracle| {info.get('gamma', float('nan')):.3e} "
          f"worst error/bar {ratio:.3f}, largest mass on a dead state {dead:g}")
    DECODE.append({"kind": "posterior", "ft": "f64" if d.dbl else "f32", "seed": seed, "ratio": ratio, "flag": int(flag), "dead": dead,
                   "redrawn": int(d.redrawn)})
    assert ratio <= 1.0, msg
    assert dead == 0.0, "posterior mass on a dead state"
    if forced:  # the forward leg's by-product is the no-gradient call's ll (tests/test_decode_fuzz.py)
        ll_ng = eng.run(P, inds, d.W, grad=False)
        assert bool(((a[0] - ll_ng).abs() <= 1e-12 * ll_ng.abs()).all()), (a[0], ll_ng)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_DECODE))
def test_viterbi(seed):
    import torch

    d = mm.decode_draw(seed, "viterbi")
    o = df.oracle_viterbi(d)
    kern, eng, pp, P, inds = tdf._setup(d)
    lens_t = None if d.lens is None else torch.as_tensor(d.lens, dtype=torch.int64).cuda()

    def call():
        if d.raw:
            return eng.viterbi(P, inds, d.W, lens=lens_t)
        return kern.viterbi(pp, d.inds, lens=d.lens)

    a, flag = _decode_calls(d, eng, call)
    logp, path = a[0].cpu().numpy(), a[1].cpu().numpy()
    ratio, msg, info = df.compare_viterbi(o, {"logp": logp, "path": path}, d)
    visits = dead_visits(d, path) if path.shape == (d.B, d.S, d.L - d.W) else -1
    unique = int(np.isinf(o["margin"]).sum())
    print(f"massless viterbi {d.describe()}: flag={int(flag)} {info.get('n_diff', -1)} sites differ, deficit {info.get('deficit', float('nan')):.3e}, "
          f"worst error/bar {ratio:.3f}, {visits} visits to a dead state, {unique} sequences with a unique path")
    DECODE.append({"kind": "viterbi", "ft": "f64" if d.dbl else "f32", "seed": seed, "ratio": ratio, "flag": int(flag), "dead": visits,
                   "unique": unique})
    assert np.isfinite(logp).all(), "logp not finite"
    assert ratio <= 1.0, msg
    assert visits == 0, "a path visits a dead state"
    assert path_mismatch_where_unique(d, o, path) == [], "the only path of positive probability was not found"
