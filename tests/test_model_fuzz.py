"""The likelihood and gradient kernels on seeded random draws over MODEL space (tests/model_fuzz.py) against the float64 oracle.

CPU: the draw itself -- every regime occurs, the blocks are what their tags say by the kernels' own predicates, the steep cases
hold a block of eight sites the hot sweep body may not run unscaled, the oracle is finite on every case.  GPU: per draw the
gradient call and the no-gradient call of one kernel object, held to the bars of test_random_shapes_against_the_oracle (ll) and
to its gradient metric applied to theta * d ll / d theta, the form every consumer of the gradient uses (see ``_run_case``).
``pytest -s -m gpu tests/test_model_fuzz.py`` prints one ``model fuzz`` line per draw; with PHK_MODEL_FUZZ_REPORT=<file> the
per-regime summary of the run is written there.
"""

from __future__ import annotations

import collections
import ctypes
import os
import warnings

import numpy as np
import pytest

import model_fuzz as mf
from parity_bars import F32_BLOCK_LL_PER_SITE, F32_GRAD_FULL, F32_GRAD_OWN, F64_GRAD_FULL, F64_GRAD_OWN, grad_error_ratios

DEFAULT_SEEDS = 96
N_SEEDS = int(os.environ.get("PHK_MODEL_FUZZ_SEEDS", str(DEFAULT_SEEDS)))
# tags every one of which must come up at least MIN_PER_TAG times over the default seeds
REGIME_TAGS = mf.REGIMES + ("unfoldable-a", "unfoldable-b", "unfoldable-c", "mixed", "mixed-fold", "dlog", "f32-block", "dense16",
                            "per-chunk", "mask-runs")
MIN_PER_TAG = 6
# draws of the 2,000-seed soak that found something, kept by name whatever the number of seeds run: name -> seed
REGRESSIONS = {
    # K = 16 float32, one-state-per-lane forward kernel on a wave whose sequences share their row (scalar-code path), emis1 = 1e-6
    # on runs of hets: a rescale after four hets took 2^-80 out, passed the DEFERRED risk threshold (2^-96), and the sweep returned
    # NaN gradients (and, through the first-order correction, a NaN ll) with the flag clear.  Such rescales are now held to
    # RISK_EXP like the groups of four of the wave-vote path: the call is flagged and accurate once repeated at interval 1.
    "nan_with_clear_flag_short_rows": 1028,
    "nan_with_clear_flag_long_rows": 1268,
    "nan_with_clear_flag_hybrid": 1688,
    "nan_with_clear_flag_plugin_surface": 808,
    # a float32 block on a float32 kernel object, 513 sites: 2.1e-5 from the oracle (F32_BLOCK_LL_PER_SITE)
    "float32_block_ll": 1255,
    # the draw itself failed: two odd particles asked of a batch of one
    "huge_regime_batch_of_one": 259,
}


def _defaults():
    return [mf.draw(seed) for seed in range(DEFAULT_SEEDS)]


# ------------------------------------------------------------------------------------------------- CPU: the draw
def test_every_regime_occurs():
    n = collections.Counter()
    for d in _defaults():
        n.update(d.tags)
    print(sorted(n.items()))
    for tag in REGIME_TAGS:
        assert n[tag] >= MIN_PER_TAG, (tag, n[tag])
    for name, _ in mf.THRESHOLDS:
        assert n[f"emis0={name}"] >= 3, name
    for e1 in mf.STEEP_EMIS1:
        assert n[f"emis1={e1:g}"] >= 3, e1
    odd_among_others = [d for d in _defaults() if d.form == "b" and d.K == 16 and not d.dbl]
    assert len(odd_among_others) >= 4
    for d in odd_among_others:
        assert d.B >= 5 and len(d.odd) == 1
    # both sides of the boundary in the float32 kernels, where the predicate exists twice (kernels and phk_prefold)
    for name, _ in mf.THRESHOLDS:
        assert any(f"emis0={name}" in d.tags and not d.dbl and not d.f32_block for d in _defaults()), name


def test_blocks_are_what_their_tags_say():
    lim = np.float32(2.0 ** -64)
    for d in _defaults():
        e0_32 = d.P[..., 4, :].astype(np.float32)
        unfoldable = (e0_32 <= lim).any(-1)  # [B, Sp]
        if d.regime == "unfoldable":
            assert unfoldable.any(), d.describe()
            if d.form == "a":
                assert unfoldable.all(), d.describe()
            elif d.form == "b":
                assert unfoldable[d.odd[0]].all() and unfoldable.sum() == unfoldable[d.odd[0]].size, d.describe()
            else:
                b, s = d.odd[0], d.flip_chunk
                assert d.per_chunk and not unfoldable[b, s] and unfoldable[b, s + 1] and unfoldable.sum() == 1, d.describe()
        if d.regime == "wide" and "foldable" in d.tags:
            assert not unfoldable.any(), d.describe()
        if d.regime == "huge":
            m = d.P[d.odd][..., 4, :].min(-1)
            assert (m > 2.0 ** -64).all() and (m < 1e-6).all() and "foldable" in d.tags, d.describe()
            miss = d.data[d.inds] == -1  # a run of at least four missing sites in a row the call uses
            assert (miss[:, :-3] & miss[:, 1:-2] & miss[:, 2:-1] & miss[:, 3:]).any(), d.describe()
        if d.regime == "threshold":
            for b in d.odd:
                assert (d.P[b, :, 4, -1] == d.threshold).all() and (d.P[b, :, 5, -1] == 1.0 - d.threshold).all()
            # the float32 kernels fold 2^-63 only; the float64 kernels also the float64 value just above 2^-64
            assert mf.folds32(d.P).all() == (d.threshold == 2.0 ** -63), d.describe()
            assert mf.folds64(d.P).all() == (d.threshold > 2.0 ** -64), d.describe()
        if d.regime in ("steep", "threshold", "huge") or d.form in ("b", "c"):
            others = [b for b in range(d.B) if b not in d.odd]
            assert (d.P[others][..., 4, :] >= 0.5).all(), d.describe()  # the rest of the batch is ordinary
        assert ("mixed-fold" in d.tags) == (d.folds().any() and not d.folds().all())
    assert np.float32(mf.ABOVE_FOLD_MIN) == lim and mf.ABOVE_FOLD_MIN > 2.0 ** -64


def test_steep_cases_hold_a_block_the_hot_body_may_not_run():
    """a T = 8 block over which the oracle's forward mass drops by more than 2^64 (HOT_BLOCK_MIN_EXP_F32 = -64), on a row the
    call uses, under a particle that has the steep emissions -- and under an ordinary particle of the same batch it does not"""
    for d in _defaults():
        if d.regime != "steep":
            continue
        ex = mf.block_mass_exponents(d.P[d.odd[0], 0], d.data[d.steep_row])
        assert ex.min() < -64.0, (d.describe(), ex.min())
        assert d.steep_row in d.inds
        others = [b for b in range(d.B) if b not in d.odd]
        assert others, d.describe()
        assert mf.block_mass_exponents(d.P[others[0], 0], d.data[d.steep_row]).min() > -64.0 + 8.0


def test_the_oracle_is_finite_on_every_case():
    for d in _defaults() + [mf.draw(seed) for seed in REGRESSIONS.values()]:
        o = mf.oracle(d)
        assert o["ll"].shape == (d.B, d.S) and np.isfinite(o["ll"]).all(), d.describe()
        assert np.isfinite(o["g"]).all(), d.describe()
        assert o["g_full"] is None or np.isfinite(o["g_full"]).all(), d.describe()
        assert (d.data.max(axis=1) > -1).all()
    assert mf.draw(3) is mf.draw(3) and np.array_equal(mf._draw(3).P, mf.draw(3).P)  # deterministic


# ------------------------------------------------------------------------------------------------- GPU
RECORDS: list[dict] = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("PHK_MODEL_FUZZ_REPORT")
    if path and RECORDS:
        with open(path, "w") as f:
            f.write(summary(RECORDS))


def summary(records):
    """per regime and float type: draws, worst ll error (absolute; and as a multiple of its bar), worst gradient err/bound in the
    theta * d/dtheta form, worst raw-form ratio (whole batch; particles whose smallest emis0 is >= 0.5), how often the flag was raised"""
    out = [f"model-space fuzz: {len(records)} draws, {sum(1 for r in records if r['failures'])} over a bar\n",
           f"{'regime':<12}{'type':<5}{'draws':>6}{'ll err':>11}{'ll/bar':>9}{'nograd/bar':>11}{'kern/bar':>9}{'err/bound':>10}"
           f"{'raw (all)':>11}{'raw (e0>=.5)':>13}{'flag':>6}{'flag@1':>7}\n"]
    for regime in mf.REGIMES:
        for ft in ("f32", "f64"):
            rs = [r for r in records if r["regime"] == regime and r["ft"] == ft]
            if not rs:
                continue
            mx = lambda k, rs=rs: max((r[k] for r in rs if r[k] == r[k]), default=float("nan"))  # noqa: E731
            raw_ok = mx("raw_ord")
            out.append(f"{regime:<12}{ft:<5}{len(rs):>6}{mx('ll_err'):>11.2e}{mx('ll'):>9.3f}{mx('nograd'):>11.3f}{mx('kern'):>9.3f}"
                       f"{mx('grad'):>10.3f}{mx('raw'):>11.2e}{raw_ok:>13.3f}{sum(r['flag'] for r in rs):>6}{sum(r['flag1'] for r in rs):>7}\n")
    fb = [r for r in records if r["f32_block_per_site"] == r["f32_block_per_site"]]
    if fb:
        w = max(fb, key=lambda r: r["ll_plain_bar"])
        out.append(f"float32 blocks on float32 kernels: {len(fb)} draws, worst |ll error| per site {max(r['f32_block_per_site'] for r in fb):.2e}, "
                   f"worst multiple of the corrected call's bar {w['ll_plain_bar']:.3f} (seed {w['seed']}, {w['ll_err']:.2e})\n")
    for r in records:
        if r["failures"]:
            out.append(f"OVER seed={r['seed']}: {'; '.join(r['failures'])}\n")
    return "".join(out)


def _ll_ratio(ll, ref, dbl, L, uncorrected=False):
    """the ll bar of test_random_shapes_against_the_oracle for a gradient call, as |error| / (atol + rtol |ref|); ``uncorrected``:
    a float32 kernel object handed a float32 block (F32_BLOCK_LL_PER_SITE)"""
    rtol, atol = (1e-10, 1e-10) if dbl else (1e-5, 1e-5 if L <= 1025 else 2e-8 * L)
    if uncorrected and not dbl:
        atol = max(1e-5, F32_BLOCK_LL_PER_SITE * L)
    return float((np.abs(ll - ref) / (atol + rtol * np.abs(ref))).max())


def _nograd_ratio(ll0, ll, dbl, L):
    """... and of its no-gradient call against its gradient call"""
    rtol, atol = (1e-12, 1e-9) if dbl else (1e-6, max(2e-5, 1e-7 * L))
    return float((np.abs(ll0 - ll) / (atol + rtol * np.abs(ll))).max())


def _engine(d, dbl=None):
    from phlash_amd.engine import HipEngine

    if d.mask_runs is not None:
        os.environ["PHK_MASK_RUNS"] = d.mask_runs  # (read when the kernel object is created)
    try:
        eng = HipEngine(d.K, d.data, double_precision=d.dbl if dbl is None else dbl)
    finally:
        os.environ.pop("PHK_MASK_RUNS", None)
    return eng


def _apply_plan(eng, plan):
    if plan[0] == "variant":
        eng.set_variant(plan[1], plan[2])
    elif plan[0] == "plan":
        eng.set_plan(plan[1], R=plan[2], T=plan[3], R_forward=plan[4], R_scan=plan[5])


def _calls(eng, d, plan):
    """the gradient call, then the no-gradient call on the same kernel object -> ll, g (float64), flag, ll0, flag0"""
    import torch

    dev = "cuda"
    p = torch.tensor(d.P.astype(np.float32) if d.f32_block else d.P, device=dev)
    inds = torch.tensor(d.inds, dtype=torch.int64, device=dev)
    if plan[0] == "hybrid":
        os.environ["PHK_HYBRID"] = plan[1]
    try:
        ll, g = eng.run(p, inds, warmup=d.W, grad=True, dlog=d.dlog)
        torch.cuda.synchronize()
        flag = eng.underflow_risk()
        ll0 = eng.run(p, inds, warmup=d.W, grad=False)
        torch.cuda.synchronize()
        flag0 = eng.underflow_risk()
    finally:
        os.environ.pop("PHK_HYBRID", None)
    return ll.cpu().numpy(), g.double().cpu().numpy(), flag, ll0.cpu().numpy(), flag0


def _grad_ratios(d, g, dbl):
    """-> (err/bound of theta * d ll / d theta, err/bound of the raw d ll / d theta, the same over the ordinary particles only); the
    raw figures are NaN for a dlog call.

    The kernels return d/db = emis0 .* d/db' etc. of the folded model, and their emis0 row is a remainder (total mass - het -
    missing): for a state with emis0 ~ 1e-15 the raw entry is rounding noise divided by emis0, and every consumer -- the chain
    rule through the parameter map, phk_ll_first_order -- multiplies it by emis0 again.  So the rows are judged as theta * d ll /
    d theta (what a dlog call returns), with the metric and the (a, c) of the random-shape test applied to the oracle's rows in
    that form; the pi row is then already pi_i * d ll / d pi_i, hence the block of ones handed to the metric."""
    o = mf.oracle(d)
    Pm = np.broadcast_to(d.P_model, g.shape)
    a, c = (F64_GRAD_OWN, F64_GRAD_FULL) if dbl else (F32_GRAD_OWN, F32_GRAD_FULL)
    g_full_d = None if o["g_full"] is None else o["g_full"] * Pm
    ones = np.ones_like(Pm)
    r_dlog = grad_error_ratios(g if d.dlog else g * Pm, o["g"] * Pm, g_full_d, ones, a, c)[0]
    if d.dlog:
        return r_dlog, float("nan"), float("nan")
    r_raw = grad_error_ratios(g, o["g"], o["g_full"], Pm, a, c)[0]
    # ... and the raw form particle by particle for the ordinary particles (every emis0 >= 0.5) of the batch, mixed or not: there it
    # is the metric of the random-shape test, and it is these particles a wrong wave vote would hurt
    r_ord = [grad_error_ratios(g[b:b + 1], o["g"][b:b + 1], None if o["g_full"] is None else o["g_full"][b:b + 1], Pm[b:b + 1], a, c)[0]
             for b in range(d.B) if d.P_model[b, :, 4, :].min() >= 0.5]
    return r_dlog, r_raw, max(r_ord, default=float("nan"))


def _prefold_forms(d):
    """``phk_prefold`` on the unrounded block -> per block: does crel have the folded form, the fallback form, or neither"""
    import torch

    from phlash_amd import _lib as L

    lib = L.load()
    Pn = d.P.reshape(-1, 7, d.K)
    n = Pn.shape[0]
    p64 = torch.tensor(Pn, device="cuda")
    p32 = torch.empty((n, 7, d.K), dtype=torch.float32, device="cuda")
    pf = torch.empty((n, 5, d.K), dtype=torch.float32, device="cuda")
    crel = torch.empty((n, 7, d.K), dtype=torch.float64, device="cuda")
    L.check(lib.phk_prefold(0, d.K, p64.data_ptr(), n, p32.data_ptr(), pf.data_ptr(), crel.data_ptr(),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    crel = crel.cpu().numpy()
    b, dd, u, v, e0, e1, pi = (Pn[:, r] for r in range(7))

    def res(x):  # relative residual of one rounding to float32
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(x != 0, (x - x.astype(np.float32).astype(np.float64)) / x, 0.0)

    em = res(1.0 / e0)
    folded = np.stack([res(e0 * b) + em, res(e0 * dd) + em, res(u), res(e0 * v) + em, -em, res(e1 / e0) - em, res(pi)], 1)
    fallback = np.stack([res(Pn[:, r]) for r in range(7)], 1)
    close = lambda x, y: np.isclose(x, y, rtol=1e-12, atol=1e-22).all(axis=(1, 2))  # noqa: E731
    assert not close(folded, fallback).any()  # the two forms can be told apart on every block
    return close(crel, folded), close(crel, fallback)


def _run_case(d):
    rec = {"seed": d.seed, "regime": d.regime, "ft": "f32" if d.dbl is False else "f64", "failures": [], "kern": float("nan"),
           "min_e0": float(d.P_model[..., 4, :].min())}
    fail = rec["failures"].append
    o = mf.oracle(d)
    eng = _engine(d)
    eng.set_rescale_interval(d.nrm)
    if "dense16" in d.tags:
        eng.set_autotune(False)
    _apply_plan(eng, d.plan)
    ll, g, flag, ll0, flag0 = _calls(eng, d, d.plan)
    rec["flag"], rec["flag1"], nrm = int(flag or flag0), 0, d.nrm
    if flag or flag0:
        # a raised flag says: the results of this call are not to be trusted, evaluate again with per-site rescaling
        if d.nrm == 1:
            fail(f"flag raised at interval 1 (gradient call {flag}, no-gradient call {flag0})")
        eng.set_rescale_interval(1)
        nrm = 1
        ll, g, f1, ll0, f01 = _calls(eng, d, d.plan)
        rec["flag1"] = int(f1 or f01)  # (recorded, not asserted)
    rec["ll_err"] = float(np.abs(ll - o["ll"]).max())
    rec["ll"] = _ll_ratio(ll, o["ll"], d.dbl, d.L, uncorrected=d.f32_block)
    rec["ll_plain_bar"] = _ll_ratio(ll, o["ll"], d.dbl, d.L)  # (recorded: against the bar of a corrected call)
    rec["f32_block_per_site"] = rec["ll_err"] / d.L if (d.f32_block and not d.dbl) else float("nan")
    rec["nograd"] = _nograd_ratio(ll0, ll, d.dbl, d.L)
    rec["grad"], rec["raw"], rec["raw_ord"] = _grad_ratios(d, g, d.dbl)
    if not np.isfinite(g).all():
        fail("gradient not finite")
    if not rec["ll"] <= 1.0:
        fail(f"ll {rec['ll']:.3f} x its bar (worst |error| {rec['ll_err']:.3e})")
    if not rec["nograd"] <= 1.0:
        fail(f"no-gradient call {rec['nograd']:.3f} x its bar from the gradient call")
    if not rec["grad"] < 1.0:
        fail(f"theta * d ll / d theta: error {rec['grad']:.3f} x its bound")
    if rec["raw_ord"] == rec["raw_ord"] and not rec["raw_ord"] < 1.0:
        fail(f"d ll / d theta of the ordinary particles: error {rec['raw_ord']:.3f} x its bound")
    if d.B * d.S >= 2:  # once through the plugin surface: the redo of a flagged call happens inside it
        from phlash_amd.kernel import get_kernel
        from phlash_amd.params import PSMCParams

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            kern = get_kernel(d.K, d.data, d.dbl, overlap=d.W)  # (the warm-up prefix of the call: run, not scored)
            kern._eng.set_rescale_interval(d.nrm)
            pp = PSMCParams(*(np.ascontiguousarray(d.P_model[:, :, r, :]) for r in range(7)))
            ll_k, _ = kern(pp, d.inds, grad=True)
        rec["kern"] = _ll_ratio(np.asarray(ll_k), o["ll"], d.dbl, d.L)
        if not rec["kern"] <= 1.0:
            fail(f"PSMCKernel.__call__: ll {rec['kern']:.3f} x its bar")
    if d.regime == "threshold":
        is_folded, is_fallback = _prefold_forms(d)
        want = mf.folds32(d.P).reshape(-1)
        if not (np.array_equal(is_folded, want) and np.array_equal(is_fallback, ~want)):
            fail(f"phk_prefold: crel folded {is_folded.tolist()} fallback {is_fallback.tolist()}, the float32 kernels fold {want.tolist()}")
    RECORDS.append(rec)
    print(f"model fuzz {d.describe()}: flag={rec['flag']} flag@1={rec['flag1']} ran nrm={nrm} ll {rec['ll']:.3f} nograd {rec['nograd']:.3f} "
          f"kern {rec['kern']:.3f} err/bound {rec['grad']:.3f} raw {rec['raw']:.3g} raw(ordinary) {rec['raw_ord']:.3g} min emis0 {rec['min_e0']:.2e}")
    assert not rec["failures"], (d.describe(), rec["failures"])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_model_space_against_the_oracle(seed):
    """Seeded random draws over what the kernels branch on in the parameter block -- folding, the wave votes on folding and on
    steep blocks, the underflow flag, folded ratios up to 2^64 -- and over the two input forms the other fuzz tests never draw
    (dlog output, a float32 parameter tensor), each against the float64 oracle on the model the call was handed.  The property
    under test: a call whose underflow flag stays clear is accurate, for every kernel family; a call that raises it is accurate
    once repeated with per-site rescaling."""
    _run_case(mf.draw(seed))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REGRESSIONS))
def test_regressions(name):
    _run_case(mf.draw(REGRESSIONS[name]))
