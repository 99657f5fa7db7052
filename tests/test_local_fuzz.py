"""The local likelihood-ratio scan (phk_local_ratio) on seeded random draws (tests/local_fuzz.py) against its float64 oracle.

CPU: what the bars need from the references alone (the float32 redraw share, the float32 emulation inside its own bars, the
structured float64 statement within the project's float64 bar on every sequence), the coverage of the default seeds, and the
comparator against the oracle's own output with one fault injected.  GPU: one call per draw through ``PSMCKernel.local_ratio``
or the raw ``HipEngine.local_ratio``, held to the comparator, to bitwise repeatability, to the gradient call's bits and plan
around it, and to ``phk_posterior``'s ll.
``pytest -s -m gpu tests/test_local_fuzz.py`` prints one ``fuzz`` line per draw and a summary (profiles/local_fuzz.txt).
"""

from __future__ import annotations

import os
import time
import warnings

import numpy as np
import pytest

import decode_fuzz as df
import local_bars
import local_fuzz as lf
import test_decode_fuzz as tdf
import test_sweep_fuzz as tsf

DEFAULT_SEEDS = 76  # the smallest count that draws the whole list of test_default_seeds_cover_the_list (seed 75 is the first
# with a block per sequence under slabs of particles); that test checks that no smaller count does
# draws that found a bug, kept by name whatever the number of seeds run: name -> seed
REGRESSIONS: dict = {}
N_SEEDS = int(os.environ.get("PHK_LOCAL_FUZZ_SEEDS", str(DEFAULT_SEEDS)))


def _defaults():
    return [lf.draw(seed) for seed in range(DEFAULT_SEEDS)]


# ------------------------------------------------------------------------------------------------- CPU
def _emulated(d):
    """the float32 emulation's output in the form of a call's"""
    o = lf.oracle(d)
    R = np.array([[o["seq"][b][s]["ratio32"] for s in range(d.S)] for b in range(d.B)]).reshape(d.B, d.S, d.nbin)
    return {"ll": o["ll"], "dtype": "float32", "log_ratio": R}


def test_reference_alone_conditions():
    """The bars are derived from the references: this is where they are checked against the references, without a kernel.
    Float32 draws that float32 itself cannot hold are redrawn as float64 -- at most 5 % of them; the float32 emulation sits
    inside its own bars; the structured float64 statement stays within F64_LOCAL_BAR of the dense oracle on every sequence of
    every float64 draw (so no float64 bar is above 10 x the project's) and agrees with it on every -inf."""
    draws = _defaults()
    f32_default = [d for d in draws if not (d.seed // 10) % 2]
    redrawn = [d.seed for d in f32_default if d.redrawn]
    kept = [d for d in draws if not d.dbl]
    worst = max(kept, key=lambda d: lf.oracle(d)["redraw"])
    print(f"local: {len(redrawn)} of {len(f32_default)} float32 draws redrawn as float64 (seeds {redrawn}); largest 5 x E kept is "
          f"{lf.oracle(worst)['redraw']:.3f} of its cap (seed {worst.seed}, alt {worst.alt_form})")
    assert len(redrawn) <= 0.05 * len(f32_default), redrawn
    top = 0.0
    for d in kept:
        if d.alt_form == "same":  # (the exact 0 belongs to the kernel's form: a dense statement steps q and beta through
            continue              # different products, and the structured one is held to it in tests/test_local_ratio.py)
        ratio, msg, _ = lf.compare(lf.oracle(d), _emulated(d), d)
        assert ratio <= 1.0, (lf.describe(d), msg)
        top = max(top, ratio)
    print(f"local: the float32 emulation on {len(kept)} float32 draws: worst ratio to its bars {top:.3f}")
    worst_s, at = 0.0, None
    for d in draws:
        if d.dbl:
            for row in lf.oracle(d)["seq"]:
                for o in row:
                    assert o["S"] <= local_bars.F64_LOCAL_BAR, (lf.describe(d), o["S"])
                    if o["S"] > worst_s:
                        worst_s, at = o["S"], d
    print(f"local: the structured statement on {sum(d.dbl for d in draws)} float64 draws: worst S / F64_LOCAL_BAR "
          f"{worst_s / local_bars.F64_LOCAL_BAR:.3f}" + (f" (seed {at.seed}, alt {at.alt_form})" if at is not None else ""))


def _alt_differs(d, axis):
    """the alternative blocks along ``axis`` (0: particles, 1: chunk positions) all differ from the first"""
    x = np.moveaxis(np.stack(d.alt[:6]), 1 + axis, 0)  # (pi is never read)
    return len(x) > 1 and all(not np.array_equal(x[0], x[i]) for i in range(1, len(x)))


def _informative(d):
    """twenty scored sites or more whose log ratio depends on the alternative block"""
    return d.L - d.W >= 20 and (d.het > 0 or d.alt_form not in ("same", "tiny_het", "dead_het"))


def _features(d):
    f = tsf._features(d)  # (the posterior draw's list and the sweeps' lens features)
    ft = "f64" if d.dbl else "f32"
    f.add(f"alt {d.alt_form} {ft}")
    by_b = d.alt_layout in ("particle", "both") and _alt_differs(d, 0) and _informative(d)
    by_s = d.alt_layout in ("chunk", "both") and _alt_differs(d, 1) and _informative(d)
    if d.alt_layout == "one" or (d.alt_layout == "particle" and by_b) or (d.alt_layout == "chunk" and by_s) or (by_b and by_s):
        f.add(f"layout {d.alt_layout}")
    Ba, Sa = d.alt.d.shape[:2]
    if (Ba > 1 or d.alt_layout in ("one", "chunk")) and (Sa > 1 or d.alt_layout in ("one", "particle")):
        f.add(f"layout {d.alt_layout} {'raw' if d.raw else 'api'}")  # (the call form sees the shape, whatever the blocks hold)
    if by_s and d.ws == "chunks":
        f.add(f"layout {d.alt_layout} under slabs of chunks")
    if by_b and d.ws == "particles":
        f.add(f"layout {d.alt_layout} under slabs of particles")
    if d.K not in df.COMPILED_K and d.plan is not None:
        f.add(f"padded K={d.K} under a forced plan")
        if d.plan[0] == "segmented":
            f.add("padded K under a forced segmented plan")
    if d.L < 8 and d.W < d.L:
        f.add("L below a block")
    if d.nbin:
        R = lf.oracle_candidate(d)["log_ratio"]
        fin = np.isfinite(R)
        if not d.dbl and (R[fin] > lf.F32_LINEAR).any():
            f.add("f32 finite bin above +88.8")
        if not d.dbl and (R[fin] < -lf.F32_LINEAR).any():
            f.add("f32 finite bin below -88.8")
        own = np.array([[o["cnt"] > 0 for o in row] for row in lf.oracle(d)["seq"]])
        if (np.isneginf(R).any(-1) & (fin & own).any(-1)).any():
            f.add("a row with -inf and finite bins")
        if d.alt_form in ("tiny_het", "indicator") and (fin & (R != 0)).any():
            f.add(f"a finite answer from an unfolded alternative {ft}")
        if d.lens is not None and d.bin > 1 and any(d.row_len(s) < d.L and (d.row_len(s) - d.W) % d.bin for s in range(d.S)):
            f.add("a lens cut inside a bin")
    return f


def _wanted():
    want = tsf._wanted("local")
    want |= {f"alt {a} {t}" for a in lf.ALT_FORMS for t in ("f32", "f64")}
    want |= {f"padded K={K} under a forced plan" for K in df.KS if K not in df.COMPILED_K}
    want |= {f"layout {x}" for x in lf.ALT_LAYOUTS} | {f"layout {x} {c}" for x in lf.ALT_LAYOUTS for c in ("raw", "api")}
    want |= {"layout chunk under slabs of chunks", "layout both under slabs of chunks", "layout particle under slabs of particles",
             "layout both under slabs of particles", "padded K under a forced segmented plan", "L below a block",
             "f32 finite bin above +88.8", "f32 finite bin below -88.8", "a row with -inf and finite bins",
             "a finite answer from an unfolded alternative f32", "a finite answer from an unfolded alternative f64",
             "a lens cut inside a bin"}
    return want


def first_covering_count(limit=128):
    """the smallest number of seeds whose draws cover the list (None: more than ``limit``)"""
    want, seen = _wanted(), set()
    for seed in range(limit):
        seen |= _features(lf.draw(seed))
        if not want - seen:
            return seed + 1
    return None


def test_default_seeds_cover_the_list():
    seen = set()
    for d in _defaults():
        seen |= _features(d)
    want = _wanted()
    assert not want - seen, f"the default seeds never draw: {sorted(want - seen)}"
    assert DEFAULT_SEEDS <= 128
    assert first_covering_count(DEFAULT_SEEDS) == DEFAULT_SEEDS, "DEFAULT_SEEDS is not the smallest count that covers the list"


def _first(pred):
    for d in _defaults():
        if pred(d):
            return d
    raise AssertionError("no default draw fits: change the draw")


def _private(d, **kw):
    """a copy of the draw with fields changed (the cached draws stay as they are)"""
    c = lf._draw(d.seed, d.dbl and d.redrawn)
    assert c.dbl == d.dbl
    for k, v in kw.items():
        setattr(c, k, v)
    c._oracle = None
    return c


def _ragged(d):
    """a draw (the first: float32 or float64) with rows that differ, own lengths that differ by row and by position, an alternative of another model"""
    return (d.S >= 2 and len(np.unique(d.inds)) >= 2 and d.L - d.W >= 20 and d.lens is not None
            and any(int(d.lens[s]) != d.row_len(s) for s in range(d.S))
            and any(d.row_len(s) < d.L and d.data[d.inds[s], d.row_len(s)] >= 0 for s in range(d.S))  # (an observed site past it)
            and d.alt_form in ("theta4", "theta_quarter", "rho_quarter", "ne2", "other", "blockout", "indicator") and d.het > 0)


def test_comparators_catch_seeded_faults():
    """The oracle's own output passes on every default draw; with one fault injected it fails.  Float32 draws where there is a
    choice: the looser bars."""
    caught = []

    def check(d, name, cand):
        ratio, msg, _ = lf.compare(lf.oracle(d), cand, d)
        print(f"local fault '{name}' on seed {d.seed}: ratio {ratio:.3g} ({msg})")
        assert ratio > 1.0, name
        caught.append(name)

    def good_of(d):
        good = lf.oracle_candidate(d)
        assert lf.compare(lf.oracle(d), good, d)[0] <= 1.0
        return good

    def edited(good, edit):
        R = good["log_ratio"].copy()
        edit(R)
        return dict(good, log_ratio=R)

    d = _first(_ragged)
    if d.bin > 16:
        d = _private(d, bin=7)
    good = good_of(d)
    check(d, "bins shifted by one site", lf.candidate(d, shift=1))
    check(d, "two chunks swapped", tsf._swap_chunks(good, d))
    check(d, "lens by position", lf.candidate(d, row_len=lambda s: int(d.lens[s])))
    check(d, "a site past a row's own length stepped with the alternative", lf.candidate(d, row_len=lambda s: min(d.row_len(s) + 1, d.L)))
    check(d, "the sign flipped", edited(good, lambda R: np.negative(R, out=R)))
    check(d, "float64 outputs from a float32 handle", dict(good, dtype="float64"))
    # a row whose own length leaves bins without a site of its own
    e = _first(lambda d: d.nbin and any((o["cnt"] == 0).any() for row in lf.oracle(d)["seq"] for o in row))
    good = good_of(e)
    b, s, k = [(b, s, int(np.flatnonzero(o["cnt"] == 0)[0])) for b, row in enumerate(lf.oracle(e)["seq"]) for s, o in enumerate(row)
               if (o["cnt"] == 0).any()][0]
    check(e, "an empty bin at 1e-30", edited(good, lambda R: R.__setitem__((b, s, k), 1e-30)))
    # the alternative's strides: a block per particle / per chunk position, with and without the other axis
    for layout in ("particle", "both"):
        e = _first(lambda d: d.alt_layout == layout and d.alt_form != "same" and _alt_differs(d, 0) and _informative(d))
        good_of(e)
        check(e, f"particle 0's alternative block for every particle ({layout})", lf.candidate(e, alt_of=lambda b, s: (0, e.alt_id(b, s)[1])))
    for layout in ("chunk", "both"):
        e = _first(lambda d: d.alt_layout == layout and d.alt_form != "same" and _alt_differs(d, 1) and _informative(d))
        good_of(e)
        check(e, f"chunk 0's alternative block for every chunk ({layout})", lf.candidate(e, alt_of=lambda b, s: (e.alt_id(b, s)[0], 0)))
    # slabs: the alternative's offset of the slab left out (the blocks counted from the slab's first sequence)
    for ws, axis in (("particles", 0), ("chunks", 1)):
        e = _first(lambda d: d.ws == ws and d.alt_form != "same" and _alt_differs(d, axis) and _informative(d))
        good_of(e)

        def in_slab(b, s, e=e):
            b0, s0 = e.slab_origin(b, s)
            return e.alt_id(b - b0, s - s0)

        check(e, f"a slab offset missing from the alternative (slabs of {ws})", lf.candidate(e, alt_of=in_slab))
    # the range beyond float32's linear ratio
    e = _first(lambda d: not d.dbl and d.nbin and np.abs(np.where(np.isfinite(x := lf.oracle_candidate(d)["log_ratio"]), x, 0)).max() > 88.8)
    check(e, "values clipped to +-87", edited(good_of(e), lambda R: np.clip(R, -87.0, 87.0, out=R)))
    # -inf
    e = _first(lambda d: d.nbin and np.isneginf(lf.oracle_candidate(d)["log_ratio"]).any())
    good = good_of(e)
    at = tuple(np.argwhere(np.isneginf(good["log_ratio"]))[0])
    check(e, "a -inf replaced by -1e30", edited(good, lambda R: R.__setitem__(at, -1e30)))
    check(e, "a -inf replaced by NaN", edited(good, lambda R: R.__setitem__(at, np.nan)))
    fin = tuple(np.argwhere(np.isfinite(good["log_ratio"]))[0])
    check(e, "a finite bin at -inf", edited(good, lambda R: R.__setitem__(fin, -np.inf)))
    check(e, "a +inf", edited(good, lambda R: R.__setitem__(fin, np.inf)))
    # alternative = fitted
    e = _first(lambda d: d.alt_form == "same" and d.nbin)
    check(e, "alternative = fitted with one entry at the smallest subnormal", edited(good_of(e), lambda R: R.__setitem__((0, 0, 0), 5e-324)))
    assert len(caught) == 19

    for d in _defaults():
        ratio, msg, _ = lf.compare(lf.oracle(d), lf.oracle_candidate(d), d)
        assert ratio <= 1.0, (lf.describe(d), msg)


# ------------------------------------------------------------------------------------------------- GPU
STATS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if not STATS:
        return
    print("\nlocal fuzz summary (per float type)")
    for ft, rows in sorted(STATS.items()):
        w = max(rows, key=lambda r: r["ratio"])
        line = (f"  local {ft}: {len(rows)} draws, worst error/bar {w['ratio']:.3f} (seed {w['seed']}), worst raw error "
                f"{max(r.get('ratio_raw', 0.0) for r in rows):.3e}")
        if ft == "f64":
            line += f", {sum(r['redrawn'] for r in rows)} of them float32 draws redrawn as float64"
        print(line)
    print(f"  wall time of test_local_random_shapes: {sum(r['time'] for rows in STATS.values() for r in rows):.1f} s (oracles included)")


def _alt_inputs(d):
    """-> (the alternative as a device tensor [Ba, Sa, 7, K] for the raw call, as PSMCParams for the API call: fields [K],
    [B, 1, K], [S, K] or [B, S, K]; the fitted layout for alternative = fitted)"""
    import torch

    from phlash_amd.params import PSMCParams

    A = torch.stack([torch.as_tensor(a) for a in d.alt], -2)  # [Ba, Sa, 7, K]
    fields = [torch.as_tensor(a) for a in d.alt]
    if d.alt_form != "same":
        if d.alt_layout == "one":
            fields = [a[0, 0] for a in fields]
        elif d.alt_layout == "chunk":
            fields = [a[0] for a in fields]
    return A.cuda(), PSMCParams(*fields)


def _local_draw(seed, record=True):
    import torch

    t0 = time.perf_counter()
    d = lf.draw(seed)
    o = lf.oracle(d)
    kern, eng, pp, P, inds = tdf._setup(d)
    A, alt = _alt_inputs(d)
    lens_t = None if d.lens is None else torch.as_tensor(d.lens, dtype=torch.int64).cuda()
    forced = d.plan is not None
    if forced:
        eng.set_plan(1 if d.plan[0] == "segmented" else 0, *d.plan[1:])
        ll0, g0 = eng.run(P, inds, d.W, grad=True)  # a gradient call before the scan ...
        plan0 = eng.get_plan()
        if d.ws_limit is not None:
            assert eng.get_slab() == d.slab, (eng.get_slab(), d.slab)

    def call():
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            if d.raw:
                ll, r = eng.local_ratio(P, A, inds, d.W, bin=d.bin, lens=lens_t)
            else:
                ll, r = kern.local_ratio(pp, alt, d.inds, bin=d.bin, lens=d.lens)
            risk = eng.underflow_risk()
        assert not risk, "underflow flag raised on ordinary parameters"
        return ll, r

    a = call()
    assert a[0].dtype == torch.float64
    cand = {"ll": a[0].cpu().numpy(), "dtype": str(a[1].dtype).replace("torch.", ""), "log_ratio": a[1].double().cpu().numpy()}
    ratio, msg, info = lf.compare(o, cand, d)
    print(f"fuzz local {lf.describe(d)}: nbin={d.nbin} worst raw error {info.get('ratio', float('nan')):.3e} worst error/bar {ratio:.3f}")
    assert ratio <= 1.0, msg
    b = call()  # a repeat call: the same bits
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    if forced:
        ll1, g1 = eng.run(P, inds, d.W, grad=True)  # ... and after it: the same bits, the plan untouched
        assert torch.equal(ll0, ll1) and torch.equal(g0, g1)
        assert eng.get_plan() == plan0
    ll_post = eng.posterior(P, inds, d.W, bin=d.bin)[0]  # the same legs at the same plan, bin and W: ll to the bit
    assert torch.equal(a[0], ll_post), (a[0], ll_post)
    assert not eng.underflow_risk()
    if record:
        STATS.setdefault("f64" if d.dbl else "f32", []).append(
            dict(seed=d.seed, ratio=ratio, ratio_raw=info.get("ratio", 0.0), redrawn=d.redrawn, time=time.perf_counter() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_local_random_shapes(seed):
    _local_draw(seed)


@pytest.mark.gpu
def test_regression_draws():
    """every pinned draw, whatever the number of seeds run (a loop: the table may be empty, and an empty parameter list skips)"""
    for name in sorted(REGRESSIONS):
        _local_draw(REGRESSIONS[name], record=False)
