"""The sampler-side kernels -- ``phk_param_map`` / ``phk_param_map_rounded``, ``phk_log_prior``, ``phk_chain_rule``, ``phk_svgd_step`` --
on seeded random draws over particle space (tests/sampler_fuzz.py), through the C ABI with ctypes, against the float64 / longdouble
references.

CPU: the draw itself -- every branch of the particle map and every size comes up, the tags are what the oracle's own output says, the
share of candidates the admission rule rejects stays under its cap, the references are finite (autograd included) on every case, the
longdouble SVGD reference equals the loop-form oracle, the select populations are what they claim to be.  GPU: per case the checks
of DESIGN.md, "Sampler-side fuzz".  ``pytest -s -m gpu tests/test_sampler_fuzz.py`` prints one ``sampler fuzz`` line per case; with
PHK_SAMPLER_FUZZ_REPORT=<file> the summary of the run is written there (profiles/sampler_fuzz.txt is one).
"""

from __future__ import annotations

import collections
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import oracle.psmc_numpy as pn
import oracle.svgd_numpy as osv
import sampler_fuzz as sf

torch = pytest.importorskip("torch")

DEFAULT_SEEDS = 40
N_SEEDS = int(os.environ.get("PHK_SAMPLER_FUZZ_SEEDS", str(DEFAULT_SEEDS)))
MIN_PER_TAG = 3  # every branch tag of sf.BRANCH_TAGS, over the default seeds
MIN_PER_K = 4
REJECTED_CAP = 0.10
# the bars of tests/test_above_the_scan.py for sigma = 1 populations: values row-scaled, JVP row-scaled, VJP, emission and pi rows
# element-wise.  A regime is held to these times max(1, 8 x (what the two oracles differ by on that regime) / VALUE_BAR): reference
# against reference on the same particles says how well the map is conditioned there, and its Jacobian differentiates the same
# cancellations (``oracle_figures``).
VALUE_BAR, JVP_BAR, VJP_BAR, ELEMENT_BAR = 4e-13, 3e-13, 4e-12, 5e-10
PRIOR = (0.3, 0.02)  # alpha, beta
# cases that found something, kept by name whatever the number of seeds run
MAP_REGRESSIONS = {
    # c_tr = 25 (seed 0: first epoch of K = 5; seed 2: last epoch of K = 16): the kernel returned softplus(x) = x above 20 as
    # torch.nn.functional.softplus does -- and so did oracle/psmc_torch.py -- where the reference's jax.nn.softplus has no threshold:
    # c off by e^-x (5.6e-13 relative at 25, 1e-10 just above 20) and d c / d x = 1.  The two oracles parted by exactly that.
    "softplus_above_20_first_epoch": 0,
    "softplus_above_20_last_epoch": 2,
}
UPDATE_REGRESSIONS: dict[str, int] = {}


def _map_cases():
    return [sf.draw_map(seed) for seed in range(DEFAULT_SEEDS)]


def _group(label):
    return "pair" if "+" in label else label


@functools.lru_cache(maxsize=None)
def oracle_figures():
    """group of particles (ordinary, wide, every single regime, pairs) -> the largest row-scaled distance between the two oracles over
    the default seeds and the regressions"""
    fig = collections.defaultdict(float)
    for c in _map_cases() + [sf.draw_map(s) for s in MAP_REGRESSIONS.values()]:
        for b in range(c.B):
            g = _group(c.label(b))
            fig[g] = max(fig[g], c.oracles_by_particle[b])
    return dict(fig)


def bar_factor(group):
    return max(1.0, 8.0 * oracle_figures().get(group, 0.0) / VALUE_BAR)


# ------------------------------------------------------------------------------------------------- CPU: the draw of part A
def test_every_branch_and_every_size_occurs():
    import test_above_the_scan as above

    tags, ks, thetas, kinds, labels = (collections.Counter() for _ in range(5))
    for c in _map_cases():
        tags.update(c.tags)
        ks[c.K] += 1
        thetas[c.theta] += 1
        kinds[c.kind] += 1
        labels.update(c.regimes.values())
        assert 3 <= c.B <= 9 and c.X.shape == (c.B, c.P + 3)
        assert 1 <= len(c.regimes) <= 3 if c.kind == "regime" else not c.regimes
        assert len(c.regimes) < c.B or c.B == 3  # ordinary particles around the odd ones
    print(sorted(tags.items()), sorted(ks.items()), sorted(labels.items()))
    for tag in sf.BRANCH_TAGS:
        assert tags[tag] >= MIN_PER_TAG, (tag, tags[tag])
    for K in sf.KS:
        assert ks[K] >= MIN_PER_K, (K, ks[K])
    assert min(thetas[t] for t in sf.THETAS) >= 8 and kinds["wide"] == kinds["regime"] == DEFAULT_SEEDS // 2
    for name, _, _ in sf.SINGLES:
        assert any(name in lab.split("+") for lab in labels), name
    assert sum("+" in lab for lab in labels.elements()) >= 5  # pairs
    for K, pat in above.PATTERNS.items():
        assert sf.PATTERNS[K] == pat
    for K in (5, 7):  # an epoch over the first state, another over the last state only
        ep = sf.epoch_of_state(sf.PATTERNS[K])
        assert len(ep) == K and ep[0] == 0 and (ep == ep[-1]).sum() == 1 and ep[-1] != ep[0]
    assert sf.draw_map(3) is sf.draw_map(3) and np.array_equal(sf._candidate(3, sf.draw_map(3).sub).X, sf.draw_map(3).X)  # deterministic


def test_tags_are_what_the_oracle_says():
    """the tags of a case against the oracle's own output and intermediate quantities, particle by particle"""
    for c in _map_cases():
        K = c.K
        for b in range(c.B):
            x, tags, want = c.X[b], c.tags_by_particle[b], c.want[b]
            dm = pn.particle_to_dm(x, c.pat, c.theta)
            e = pn.ect(dm.t, dm.c)
            assert ("softplus>20" in tags) == bool((x[2:2 + c.P] > 20).any())
            assert ("c>100" in tags) == bool((dm.c[:-1] > 100).any()) and ("c~0" in tags) == bool(np.isclose(dm.c[:-1], 0).any())
            for k in np.nonzero(dm.c[:-1] > 100)[0]:
                assert e[k] == max(dm.t[k], 1e-20), c.describe()  # E[t_k] = t_k: the next step of the augmented grid is exactly 0
            for k in np.nonzero(np.isclose(dm.c[:-1], 0))[0]:
                assert e[k] == max((dm.t[k] + dm.t[k + 1]) / 2, 1e-20), c.describe()
            assert ("e-floor" in tags) == bool((e == 1e-20).any())
            t_aug = np.stack([dm.t, e], 1).reshape(-1)
            general = np.isclose(np.diff(t_aug), 0.0)
            general[0:2 * (K - 1):2] &= ~(dm.c[:-1] > 100)
            assert ("skip-dt" in tags) == bool(general.any())
            assert ("emis0-lo" in tags) == bool((want[4] == 1e-20).any()) and ("emis1-lo" in tags) == bool((want[5] == 1e-20).any())
            assert ("pi-lo" in tags) == bool((want[6] == 1e-20).any()) and ("b-lo" in tags) == bool((want[0, :K - 1] == 1e-20).any())
            lab = c.regimes.get(b)
            if lab is None and c.kind == "regime":  # the rest of the batch is ordinary: N(0, 0.25) around the default model
                assert not tags & {"softplus>20", "c>100", "c~0", "e-floor", "skip-dt", "emis0-lo", "emis1-lo"}, c.describe()
            for name in (lab or "").split("+"):
                if name.startswith("c25") or name.startswith("c120"):
                    assert "softplus>20" in tags
                if name.startswith("c-19"):
                    assert (x[2:2 + c.P] == -19.0).any()
                if name in ("t1-20", "t1-30"):
                    assert "skip-dt" in tags, c.describe()
        assert c.oracles <= sf.ORACLES_AGREE and c.tags == set().union(*c.tags_by_particle)


def test_rejected_share_stays_under_its_cap():
    cases = _map_cases()
    rejected = sum(len(c.rejected) for c in cases)
    share = rejected / (rejected + len(cases))
    print(f"rejected {rejected} of {rejected + len(cases)} candidates ({share:.1%}): " + "; ".join(f"{c.seed}.{s} {w}" for c in cases for s, w in c.rejected))
    assert share <= REJECTED_CAP


def test_admission_rule_rejects_a_particle_on_a_threshold():
    """what the rule is for: the default particle is admitted; the same particle with softplus(c_tr) = 100 + 5e-7 in one epoch, where
    -1e-6 on that coordinate leaves the c > 100 branch, is not"""
    pat, theta = sf.PATTERNS[16], 1e-2
    P = len(pn.parse_pattern(pat))
    x0 = pn.particle_from_linear(pat, 1e-4, 15.0, np.ones(P), theta, 2 * theta)
    case = lambda x: sf.MapCase(seed=-1, sub=0, K=16, pat=pat, P=P, theta=theta, kind="regime", regimes={}, B=1, X=np.array(x)[None])  # noqa: E731
    assert sf._admit(case(x0)) is None
    edge = np.array(x0)
    edge[4] = 100.0 + 5e-7
    assert "predicate" in (sf._admit(case(edge)) or "")


def test_references_are_finite_on_every_case():
    import oracle.psmc_torch as pt

    for c in _map_cases() + [sf.draw_map(s) for s in MAP_REGRESSIONS.values()]:
        assert np.isfinite(c.want).all() and np.isfinite(c.want_torch).all(), c.describe()
        for b in range(c.B):
            xb = torch.tensor(c.X[b], requires_grad=True)
            out = pt.particle_to_params(xb, c.pat, c.theta)
            (g,) = torch.autograd.grad(out, xb, torch.ones_like(out))  # a NaN or inf anywhere in the Jacobian shows here
            assert torch.isfinite(g).all(), (c.describe(), b)
            v = sf.log_prior_torch(xb, c.P, *PRIOR)
            (gp,) = torch.autograd.grad(v, xb)
            assert torch.isfinite(gp).all() and abs(float(v.detach()) - pn.log_prior(c.X[b], c.pat, *PRIOR)) <= 1e-12 * max(1.0, abs(float(v.detach())))


def test_the_plain_jvp_metric_is_too_tight_for_the_reference_itself():
    """The evidence behind ``jacobian_errors``: on particle 5 of seed 1 (a wide K = 7 particle whose v_k reach the 1e-20 clip) the
    oracle's own reverse-mode Jacobian, multiplied by a tangent, stands 1.8e-11 row-scaled from the oracle's own JVP -- sixty times the
    plain bar of 3e-13 -- and inside that bar against the sum of absolute terms."""
    import oracle.psmc_torch as pt

    c, b = sf.draw_map(1), 5
    fn = lambda z: pt.particle_to_params(z, c.pat, c.theta)  # noqa: E731
    xb = torch.tensor(c.X[b])
    Jr = torch.autograd.functional.jacobian(fn, xb).numpy()
    tan = np.random.default_rng([45_000, c.seed, b]).normal(size=c.P + 3)
    _, jo = torch.autograd.functional.jvp(fn, xb, torch.tensor(tan))
    jvp, _, plain, _ = jacobian_errors(Jr, tan, jo.numpy(), None, None)
    print(f"reverse-mode Jacobian x tangent against the JVP of the same oracle: plain {plain:.2e}, against absolute sums {jvp:.2e}")
    assert jvp < JVP_BAR < 10 * JVP_BAR < plain  # (measured 1.1e-13 and 1.8e-11)


# ------------------------------------------------------------------------------------------------- CPU: part B
@pytest.mark.parametrize("B,D", [(1, 4), (2, 1), (3, 2), (7, 5), (12, 18)])
def test_longdouble_reference_against_the_loop_oracle(B, D):
    """``sf.svgd_reference`` + ``sf.median_heuristic`` against oracle/svgd_numpy.py over three consecutive steps, to 1e-13"""
    rng = np.random.default_rng(B * 100 + D)
    x = rng.normal(size=(B, D))
    ref = osv.State(x)
    mu, nu, nm, h = np.zeros((B, D)), np.zeros((B, D)), np.zeros((B, D)), 1.0
    for it in range(3):
        G = rng.normal(size=(B, D)) * (1 + it)
        r = sf.svgd_reference(x, G, mu, nu, nm, h, it + 1, 0.1)
        ref = osv.step(ref, G, 0.1)
        x, mu, nu, nm = (np.asarray(r[k], dtype=np.float64) for k in ("x_out", "mu", "nu", "nu_max"))
        h = float(sf.median_heuristic(x))
        for got, want in ((x, ref.particles), (mu, ref.mu), (nu, ref.nu), (nm, ref.nu_max)):
            assert float(np.abs(got - want).max()) <= 1e-13 * max(1.0, float(np.abs(want).max()))
        assert abs(h - ref.length_scale) <= 1e-13 * ref.length_scale


def test_update_draw_covers_the_sizes_and_its_bounds_hold_for_plain_float64():
    """every D and every B, every count / lr / h_in; and the forward-error bounds of the longdouble reference are not too tight
    for correct code: the same formulas in plain float64 numpy (pairwise summation, the host's exp) stay within them"""
    cases = [sf.draw_update(seed) for seed in range(DEFAULT_SEEDS)]
    n = collections.Counter()
    for c in cases:
        n.update([("D", c.D), ("B", c.B), ("count", c.count), ("lr", c.lr), ("h", c.h_factor), ("twins", c.twins)])
        assert (c.nu >= 0).all() and (c.nu_max >= 0).all() and np.abs(c.mu).min() > 0
    for D in sf.DS:
        assert n[("D", D)] >= 5, D
    for B in sf.BS:
        assert n[("B", B)] >= 4, B
    assert min(n[("count", v)] for v in (1, 2, 1000)) >= 8 and min(n[("lr", v)] for v in (0.0, 0.1)) >= 15
    assert min(n[("h", v)] for v in (1e-3, 1.0, 1e4)) >= 8 and n[("twins", True)] >= 8
    worst = collections.defaultdict(float)
    for c in cases:
        if c.B > 17 and c.seed % 3:
            continue  # (a third of the large ones is evidence enough; each costs a second)
        r, f = c.reference(), sf.svgd_float64(c.x, c.g, c.mu, c.nu, c.nu_max, c.h_in, c.count, c.lr)
        assert all(np.isfinite(np.asarray(r[k], dtype=np.float64)).all() for k in r if k != "gamma"), c.describe()
        for k in ("mu", "nu", "nu_max", "x_out"):
            ratio = float((np.abs(f[k] - r[k]) / r["bound_" + k]).max())
            worst[k] = max(worst[k], ratio)
            assert ratio < 1.0, (c.describe(), k, ratio)
        if c.h_factor == 1e-3 and c.D >= 17 and not c.twins and c.B > 2:  # the off-diagonal kernel values underflow: d^2 / h ~ 1e3 log B
            k = np.exp(-np.asarray(sf.pairwise(c.x), dtype=np.float64) ** 2 / c.h_in)
            assert k.max() < 1e-100, c.describe()
            n[("all-zero", bool((k == 0).all()))] += 1
    assert n[("all-zero", True)] >= 3
    print("plain float64 numpy against the longdouble reference, worst error / bound:", dict(worst))


def _buckets(d):
    """the select's monotone map of [min, max] onto 2,048 buckets, as csrc/svgd_step.hip states it"""
    mn, mx = d.min(), d.max()
    scale = 2047.0 / (mx - mn)
    return np.minimum(((d - mn) * scale).astype(np.int64), 2047), scale


@pytest.mark.parametrize("kind,B,D", sf.SELECT_CASES)
def test_select_populations_are_what_they_claim(kind, B, D):
    x = sf.select_population(kind, B, D)
    assert x.shape == (B, D)
    d = np.sort(np.asarray(sf.pairwise(x), dtype=np.float64))
    if kind == "denormal":  # the float64 definition: the squares underflow
        d = np.sort(np.concatenate([np.sqrt(((x[i] - x[:i]) ** 2).sum(1)) for i in range(1, B)]))
    n = d.size
    lo, hi = (n - 1) // 2, n // 2
    bk, scale = _buckets(d)
    if kind == "outlier":
        assert (bk == 0).sum() == n - (B - 1) and (bk[-(B - 1):] >= 2046).all()
        assert ((bk == 0).sum() > 4096) and len(np.unique(d[bk == 0])) > 4096  # the narrowing path / a candidate list of nearly n
    elif kind == "clusters":
        within = d < 20.0
        assert within.sum() == lo + 1 and within[lo] and (hi == lo or not within[hi])
        assert (n % 2 == 0) == (B in (40, 300))
        if hi != lo:
            assert bk[hi] > bk[lo] + 1  # the two middle ranks in different buckets, empty ones between
        assert (bk < bk[lo]).sum() > 0  # `below` > 0
    elif kind == "line":
        u = np.unique(d)
        assert len(u) <= B - 1 + 2 * D and len(u) < n // 10  # many exact ties
        assert (np.diff(u) <= 2 * np.spacing(1.0) * math.sqrt(D)).all()  # neighbouring values one ulp of the coordinates apart
    elif kind == "denormal":
        d2 = (x[2, 0] - x[0, 0]) ** 2
        assert d2 == 2.0 ** -1074 and d[0] == 0.0 and d[1] == d[2] == 2.0 ** -537  # the square is the smallest subnormal
        if B == 3:
            assert scale == 2047.0 / 2.0 ** -537 and np.isfinite(scale) and bk.tolist() == [0, 2047, 2047]
    else:
        assert n > 32768 and (n % 2 == 0) == (B == 257)  # the chip-wide select, even and odd


# ------------------------------------------------------------------------------------------------- GPU
RECORDS: dict[str, list] = {"map": [], "update": [], "select": []}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("PHK_SAMPLER_FUZZ_REPORT")
    if path and any(RECORDS.values()):
        with open(path, "w") as f:
            f.write(summary(RECORDS))


def summary(records):
    mx = lambda rs, k: max((r[k] for r in rs), default=float("nan"))  # noqa: E731
    out = [f"sampler-side fuzz: {len({r['case'] for r in records['map']})} particle-map cases ({len(records['map'])} particles), "
           f"{len(records['update'])} update cases, {len(records['select'])} select populations\n\n",
           "particle map: worst error per group of particles, beside what the two oracles differ by there and the bar that follows\n",
           f"{'group':<12}{'particles':>10}{'oracles':>11}{'value':>11}{'bar':>10}{'JVP':>11}{'bar':>10}{'JVP/bar':>9}{'ref JVP':>10}{'JVP 60d':>10}{'VJP':>11}{'bar':>10}{'JVP plain':>11}{'VJP plain':>11}{'element':>11}{'prior':>10}{'chain':>8}\n"]
    fig = oracle_figures() if records["map"] else {}
    for g in sorted({r["group"] for r in records["map"]}):
        rs = [r for r in records["map"] if r["group"] == g]
        f = bar_factor(g)
        out.append(f"{g:<12}{len(rs):>10}{fig.get(g, 0.0):>11.2e}{mx(rs, 'value'):>11.2e}{VALUE_BAR * f:>10.1e}{mx(rs, 'jvp'):>11.2e}{JVP_BAR * f:>10.1e}{mx(rs, 'jvp_bar'):>9.3f}{mx(rs, 'jvp_ref'):>10.2e}{mx(rs, 'jvp_mp'):>10.2e}"
                   f"{mx(rs, 'vjp'):>11.2e}{VJP_BAR * f:>10.1e}{mx(rs, 'jvp_plain'):>11.2e}{mx(rs, 'vjp_plain'):>11.2e}{mx(rs, 'element'):>11.2e}{mx(rs, 'prior'):>10.2e}{mx(rs, 'chain'):>8.3f}\n")
    if records["map"]:
        out.append(f"values against the 60-digit map, row-scaled, worst: kernel {mx(records['map'], 'value_mp'):.2e}, numpy oracle {mx(records['map'], 'oracle_mp'):.2e}\n")
    out.append("(value: row-scaled; JVP, VJP: against the sum of absolute terms, see jacobian_errors; JVP/bar: against the larger of the group's bar and 8 x ref JVP = autograd against the 60-digit map on that product; JVP 60d: the kernel against the 60-digit map; plain: the metrics of test_above_the_scan.py, reported; element: emission and pi rows, error / tolerance; prior: gradient, "
               "row-scaled; chain: error / bound)\n\nSVGD / AMSGrad update: worst error / bound per quantity\n")
    for k in ("mu", "nu", "nu_max", "x_out"):
        out.append(f"  {k:<8}{mx(records['update'], k):.3f}\n")
    out.append(f"  distances {mx(records['update'], 'dist_ulp'):.2f} ulp (worst, as a share of D + 2: {mx(records['update'], 'dist'):.3f}); "
               f"h_out against the median of the distances read back {mx(records['update'], 'h_ulp'):.2f} ulp\n\nselect populations\n")
    for r in records["select"]:
        out.append(f"  {r['name']:<22}distances {r['dist_ulp']:.2f} ulp, h_out {r['h_ulp']:.2f} ulp\n")
    return "".join(out)


def _lib():
    from phlash_amd import _lib as L

    return L, L.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def jacobian_errors(J, tan, jo, cot, go):
    """-> (JVP error, VJP error, and the two in the plain metrics of tests/test_above_the_scan.py) of an entry-wise Jacobian J [7, K, D]
    against a reference product J tan [7, K] and / or J^T cot [D].

    The plain metrics divide by the largest entry of the reference PRODUCT (per row of the block for the JVP).  A product formed
    from entries each good to a few roundings errs by those roundings of sum_d |J_kd tan_d|, not of |sum_d J_kd tan_d|; for a sigma = 1
    population the two are alike, but in a row such as u_k = A[k, k+1] / v_k+1 with v_k+1 at its 1e-20 clip the entries are 1e5 and
    cancel.  The oracle's own reverse-mode Jacobian times the tangent misses the plain JVP bar there by a factor 60 against the
    oracle's own JVP (test_the_plain_jvp_metric_is_too_tight_for_the_reference_itself), so the products are judged against the sum of
    absolute terms, largest over the row (JVP) or over the coordinates (VJP), with the bars unchanged; the plain figures are reported."""
    jvp = vjp = jvp_plain = vjp_plain = 0.0
    if tan is not None:
        got = J @ tan
        scale = (np.abs(J) @ np.abs(tan)).max(-1, keepdims=True)
        jvp = float((np.abs(got - jo) / np.where(scale > 0, scale, 1.0)).max())
        jvp_plain = sf.row_scaled(got, jo)
    if cot is not None:
        g = np.einsum("rk,rkd->d", cot, J)
        scale = float(np.einsum("rk,rkd->d", np.abs(cot), np.abs(J)).max())
        vjp = float(np.abs(g - go).max() / (scale or 1.0))
        vjp_plain = float(np.abs(g - go).max() / (np.abs(go).max() or 1.0))
    return jvp, vjp, jvp_plain, vjp_plain


def _run_map_case(c):
    import oracle.psmc_torch as pt

    L, lib = _lib()
    K, P, B, D = c.K, c.P, c.B, c.P + 3
    x = _dev(c.X)
    params, params2 = (torch.full((B, 7, K), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
    jac = torch.full((B, 7 * K, D), float("nan"), dtype=torch.float64, device="cuda")
    p32 = torch.full((B, 7, K), float("nan"), dtype=torch.float32, device="cuda")
    ep = sf.epoch_of_state(c.pat)
    epp = ep.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    L.check(lib.phk_param_map_rounded(0, K, P, epp, c.theta, x.data_ptr(), B, params.data_ptr(), jac.data_ptr(), p32.data_ptr(), _stream()))
    L.check(lib.phk_param_map(0, K, P, epp, c.theta, x.data_ptr(), B, params2.data_ptr(), None, _stream()))
    got, want = params.cpu().numpy(), c.want
    J = jac.cpu().numpy().reshape(B, 7, K, D)
    failures = []
    fail = failures.append
    if not np.array_equal(params2.cpu().numpy(), got):
        fail("phk_param_map without a Jacobian differs from phk_param_map_rounded with one")
    if not np.array_equal(p32.cpu().numpy(), got.astype(np.float32)):
        fail("params_f32 is not float32(params)")
    if not (np.isfinite(got).all() and np.isfinite(J).all()):
        fail("not finite")
    # structural zeros / ones of params.py:44-55; every probability inside its clip
    if not ((got[:, 0, -1] == 0).all() and (got[:, 2, -1] == 0).all() and (got[:, 3, 0] == 0).all() and (got[:, 3, 1] == 1).all()):
        fail("structural zeros / ones")
    inside = np.ones((7, K), dtype=bool)
    inside[[2, 3]] = False
    inside[0, -1] = False
    if not ((got[:, inside] >= sf.LO) & (got[:, inside] <= 1.0)).all():
        fail("an entry of b, d, emis0, emis1 or pi outside [1e-20, 1]")
    mask = sf.clip_mask(want)
    if not (got[mask] == sf.LO).all():
        fail(f"{int((got[mask] != sf.LO).sum())} of {int(mask.sum())} entries the oracle has at the 1e-20 clip are not at it")
    if not (J[mask] == 0).all():
        fail(f"Jacobian rows of clipped entries not exactly zero ({int((J[mask] != 0).any(-1).sum())} rows)")
    # prior and chain rule on the same particles, the chain rule with the real Jacobian
    alpha, beta = PRIOR
    pv = torch.empty(B, dtype=torch.float64, device="cuda")
    pg = torch.empty((B, D), dtype=torch.float64, device="cuda")
    L.check(lib.phk_log_prior(0, P, alpha, beta, x.data_ptr(), B, pv.data_ptr(), pg.data_ptr(), _stream()))
    rng = np.random.default_rng([44_000, c.seed])
    buf = rng.normal(size=(B + 1, 1 + 7 * K)) * 50
    bad, bad_value = int(rng.integers(B)), [np.nan, np.inf, -np.inf][c.seed % 3]
    buf[bad, 0] = bad_value
    extra = c.seed % 3 == 0
    ev, eg = rng.normal(size=B), rng.normal(size=(B, D))
    c0, c1, c2 = 1.0, 37.5, 0.7
    tb, tev, teg = _dev(buf), _dev(ev), _dev(eg)
    logp = torch.empty(B, dtype=torch.float64, device="cuda")
    grad = torch.empty((B, D), dtype=torch.float64, device="cuda")
    L.check(lib.phk_chain_rule(0, K, P, alpha, beta, x.data_ptr(), tb.data_ptr(), jac.data_ptr(), B, c0, c1,
                               tev.data_ptr() if extra else None, teg.data_ptr() if extra else None, c2, logp.data_ptr(), grad.data_ptr(), _stream()))
    pv, pg, logp, grad = (t.cpu().numpy() for t in (pv, pg, logp, grad))
    if not (logp[bad] == -np.inf and (grad[bad] == 0).all()):
        fail(f"chain rule: buf[{bad}, 0] = {bad_value} gave logp {logp[bad]} and a gradient row with {int((grad[bad] != 0).sum())} non-zeros")
    for b in range(B):
        lab = c.label(b)
        f = bar_factor(_group(lab))
        rec = {"case": c.seed, "group": _group(lab), "label": lab, "oracles": c.oracles_by_particle[b]}
        rec["value"] = sf.row_scaled(got[b], want[b])
        if not rec["value"] < VALUE_BAR * f:
            fail(f"particle {b} ({lab}): values {rec['value']:.2e} row-scaled, bar {VALUE_BAR * f:.1e}")
        # emission and pi rows element-wise.  E[t_k] is formed as 1 / c + t_k - dt / expm1(c dt): terms of size 1 / c + t_k+1, so the
        # emissions carry theta x a few roundings of that absolutely; pi_k are differences of survival values <= 1, pi_0 = 1 - their sum
        dm = pn.particle_to_dm(c.X[b], c.pat, c.theta)
        t_next = np.concatenate([dm.t[1:], dm.t[-1:]])
        tol_e = ELEMENT_BAR * f * np.abs(want[b, 4:6]) + c.theta * 8 * sf.U * (1.0 / dm.c + t_next)
        tol_pi = ELEMENT_BAR * f * np.abs(want[b, 6]) + (K + 4) * sf.U
        rec["element"] = float(max((np.abs(got[b, 4:6] - want[b, 4:6]) / tol_e).max(), (np.abs(got[b, 6] - want[b, 6]) / tol_pi).max()))
        if not rec["element"] < 1.0:
            fail(f"particle {b} ({lab}): emission / pi rows element-wise {rec['element']:.3f} x their tolerance")
        # Jacobian: three JVPs, three VJPs against autograd of the torch oracle
        fn = lambda z: pt.particle_to_params(z, c.pat, c.theta)  # noqa: E731
        xb = torch.tensor(c.X[b])
        r2 = np.random.default_rng([45_000, c.seed, b])
        rec["jvp"] = rec["vjp"] = rec["jvp_plain"] = rec["vjp_plain"] = rec["jvp_ref"] = rec["jvp_mp"] = rec["jvp_bar"] = 0.0
        for i in range(3):
            tan = r2.normal(size=D)
            _, jo = torch.autograd.functional.jvp(fn, xb, torch.tensor(tan))
            jvp, _, jvp_plain, _ = jacobian_errors(J[b], tan, jo.numpy(), None, None)
            # reference against reference, for this very product: autograd against a central difference of the 60-digit map.  Where
            # c dt is in the hundreds every float64 evaluation of transition.py:9-34 loses three digits (exp(u - v)), autograd's included;
            # the bar is the larger of the group's and 8 x that figure
            val_mp, jm = sf.mp_values_and_jvp(c.X[b], c.pat, c.theta, tan)
            ref, _, _, _ = jacobian_errors(J[b], tan, jm, None, None)  # (the kernel against the 60-digit product: reported)
            scale = (np.abs(J[b]) @ np.abs(tan)).max(-1, keepdims=True)
            ref_err = float((np.abs(jo.numpy() - jm) / np.where(scale > 0, scale, 1.0)).max())
            bar = max(JVP_BAR * f, 8.0 * ref_err)
            if not jvp < bar:
                fail(f"particle {b} ({lab}): JVP {i} {jvp:.2e} against absolute sums, bar {bar:.1e} (group {JVP_BAR * f:.1e}, autograd against 60 digits {ref_err:.2e})")
            cot = r2.normal(size=(7, K))
            _, go = torch.autograd.functional.vjp(fn, xb, torch.tensor(cot))
            _, vjp, _, vjp_plain = jacobian_errors(J[b], None, None, cot, go.numpy())
            rec["jvp"], rec["vjp"], rec["jvp_ref"], rec["jvp_mp"] = max(rec["jvp"], jvp), max(rec["vjp"], vjp), max(rec["jvp_ref"], ref_err), max(rec["jvp_mp"], ref)
            rec["jvp_plain"], rec["vjp_plain"], rec["jvp_bar"] = max(rec["jvp_plain"], jvp_plain), max(rec["vjp_plain"], vjp_plain), max(rec["jvp_bar"], jvp / bar)
        rec["value_mp"], rec["oracle_mp"] = sf.row_scaled(got[b], val_mp), sf.row_scaled(want[b], val_mp)
        if not rec["vjp"] < VJP_BAR * f:
            fail(f"particle {b} ({lab}): VJP {rec['vjp']:.2e}, bar {VJP_BAR * f:.1e}")
        # prior: value against the numpy oracle, gradient against autograd of the torch restatement
        xg = torch.tensor(c.X[b], requires_grad=True)
        (ga,) = torch.autograd.grad(sf.log_prior_torch(xg, P, alpha, beta), xg)
        ga = ga.numpy()
        want_pv = pn.log_prior(c.X[b], c.pat, alpha, beta)
        rec["prior"] = float(np.abs(pg[b] - ga).max() / max(float(np.abs(ga).max()), 1e-300))
        if not abs(pv[b] - want_pv) <= 1e-12 + 1e-12 * abs(want_pv):
            fail(f"particle {b} ({lab}): log prior {pv[b]!r}, oracle {want_pv!r}")
        if not rec["prior"] < 1e-12:
            fail(f"particle {b} ({lab}): prior gradient {rec['prior']:.2e} row-scaled")
        # chain rule: (7 K + 8) roundings of the sum of absolute terms, plus the prior gradient's own bar
        rec["chain"] = 0.0
        if b != bad:
            G = buf[b, 1:].astype(np.longdouble)
            Jb = J[b].reshape(7 * K, D).astype(np.longdouble)
            want_g = c0 * ga + c1 * (G @ Jb) + (c2 * eg[b] if extra else 0.0)
            mag = np.abs(c0 * ga) + abs(c1) * (np.abs(G) @ np.abs(Jb)) + (np.abs(c2 * eg[b]) if extra else 0.0)
            bound = (7 * K + 8) * sf.U * mag + 1e-12 * abs(c0) * np.abs(ga).max() + sf.TINY
            rec["chain"] = float((np.abs(grad[b] - want_g) / bound).max())
            want_lp = c0 * want_pv + c1 * buf[b, 0] + (c2 * ev[b] if extra else 0.0)
            if not abs(logp[b] - want_lp) <= 1e-12 * abs(want_lp):
                fail(f"particle {b} ({lab}): chain rule logp {logp[b]!r}, want {want_lp!r}")
            if not rec["chain"] < 1.0:
                fail(f"particle {b} ({lab}): chain rule gradient {rec['chain']:.3f} x its bound")
        RECORDS["map"].append(rec)
        print(f"sampler fuzz map seed={c.seed} particle {b} {lab}: oracles {rec['oracles']:.2e} value {rec['value']:.2e} (bar {VALUE_BAR * f:.1e}) "
              f"jvp {rec['jvp']:.2e} (plain {rec['jvp_plain']:.2e}, autograd against 60 digits {rec['jvp_ref']:.2e}, kernel against 60 digits {rec['jvp_mp']:.2e}) vjp {rec['vjp']:.2e} (plain {rec['vjp_plain']:.2e}) element {rec['element']:.3f} prior {rec['prior']:.2e} chain {rec['chain']:.3f}")
    print(f"sampler fuzz map {c.describe()}: {'; '.join(failures) or 'ok'}")
    assert not failures, (c.describe(), failures)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_particle_map_prior_and_chain_rule(seed):
    """One admitted case through ``phk_param_map_rounded`` (values, Jacobian, the float32 copy), ``phk_param_map``, ``phk_log_prior``
    and ``phk_chain_rule``: values against the numpy oracle, the Jacobian as JVPs / VJPs against autograd of the torch oracle, clipped
    entries bit for bit with exactly zero Jacobian rows, the prior's gradient against autograd, the chain rule with the case's own
    Jacobian and one non-finite log-likelihood."""
    _run_map_case(sf.draw_map(seed))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MAP_REGRESSIONS) + sorted(UPDATE_REGRESSIONS))
def test_regressions(name):
    if name in MAP_REGRESSIONS:
        _run_map_case(sf.draw_map(MAP_REGRESSIONS[name]))
    else:
        _run_update_case(sf.draw_update(UPDATE_REGRESSIONS[name]))


def _ulps(got, ref_ld):
    """|got - ref| in units of the spacing of float64 at ref"""
    ref = np.asarray(ref_ld, dtype=np.float64)
    return float((np.abs(got.astype(np.longdouble) - ref_ld) / np.spacing(np.maximum(np.abs(ref), sf.TINY))).max()) if got.size else 0.0


def _svgd_step(x, g, mu, nu, nm, h_in, count, lr):
    """one ``phk_svgd_step`` -> (mu, nu, nu_max, x_out, h_out, the B (B - 1) / 2 distances from the front of the workspace)"""
    L, lib = _lib()
    B, D = x.shape
    tx, tg, tmu, tnu, tnm = (_dev(a) for a in (x, g, mu, nu, nm))
    th_in, th_out = _dev([h_in]), torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    x_out = torch.full((B, D), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.full((int(lib.phk_svgd_workspace_doubles(B)),), float("nan"), dtype=torch.float64, device="cuda")
    L.check(lib.phk_svgd_step(0, B, D, tx.data_ptr(), tg.data_ptr(), tmu.data_ptr(), tnu.data_ptr(), tnm.data_ptr(), th_in.data_ptr(),
                              th_out.data_ptr(), x_out.data_ptr(), ws.data_ptr(), count, lr, sf.B1, sf.B2, sf.EPS, _stream()))
    torch.cuda.synchronize()
    n = B * (B - 1) // 2
    return tuple(t.cpu().numpy() for t in (tmu, tnu, tnm, x_out)) + (float(th_out), ws[:n].cpu().numpy())


def _check_distances_and_select(x_out, dist, h_out, B, D, exact=False):
    """the distances against the longdouble reference on the kernel's own x_out, within D + 2 ulp (``exact``: bit for bit against
    float64 sqrt(fl(d^2)), for squares that underflow); h_out against the median of exactly those doubles, squared, over log B, to 4
    ulp -> (worst distance error in ulps, h_out error in ulps)"""
    if B == 1:
        assert h_out == 1.0 and dist.size == 0
        return 0.0, 0.0
    assert np.isfinite(dist).all() and (dist >= 0).all()
    if exact:
        ref = np.concatenate([np.sqrt(((x_out[i] - x_out[:i]) ** 2).sum(1)) for i in range(1, B)])
        du = 0.0 if np.array_equal(dist, ref) else float("inf")
    else:
        du = _ulps(dist, sf.pairwise(x_out))
    want_h = float(np.median(dist)) ** 2 / math.log(B)
    hu = abs(h_out - want_h) / float(np.spacing(max(want_h, sf.TINY)))
    return du, hu


def _run_update_case(c):
    r = c.reference()
    mu, nu, nm, x_out, h_out, dist = _svgd_step(c.x, c.g, c.mu, c.nu, c.nu_max, c.h_in, c.count, c.lr)
    rec, failures = {"seed": c.seed}, []
    for k, got in (("mu", mu), ("nu", nu), ("nu_max", nm), ("x_out", x_out)):
        rec[k] = float((np.abs(got.astype(np.longdouble) - r[k]) / r["bound_" + k]).max())
        if not rec[k] < 1.0:
            failures.append(f"{k}: error {rec[k]:.3f} x its bound")
    if c.lr == 0.0 and not np.array_equal(x_out, c.x):
        failures.append("lr = 0 moved the particles")
    rec["dist_ulp"], rec["h_ulp"] = _check_distances_and_select(x_out, dist, h_out, c.B, c.D)
    rec["dist"] = rec["dist_ulp"] / (c.D + 2)
    if not rec["dist"] <= 1.0:
        failures.append(f"distances {rec['dist_ulp']:.2f} ulp, D + 2 = {c.D + 2}")
    if not rec["h_ulp"] <= 4.0:
        failures.append(f"h_out {rec['h_ulp']:.2f} ulp from the median of the distances read back")
    RECORDS["update"].append(rec)
    print(f"sampler fuzz update {c.describe()}: error / bound mu {rec['mu']:.3f} nu {rec['nu']:.3f} nu_max {rec['nu_max']:.3f} x_out {rec['x_out']:.3f}, "
          f"distances {rec['dist_ulp']:.2f} ulp, h_out {rec['h_ulp']:.2f} ulp")
    assert not failures, (c.describe(), failures)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_svgd_update(seed):
    """``phk_svgd_step`` at D in {1 ... 72} and B around the distance tile and the kernel-row stride, from a running AMSGrad state,
    with count, lr and h_in varied: mu, nu, nu_max and x_out within the forward-error bounds of the longdouble reference; the
    distances of the new particles and the select judged separately (``_check_distances_and_select``)."""
    _run_update_case(sf.draw_update(seed))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B,D", sf.SELECT_CASES)
def test_median_select(kind, B, D):
    """The bucket select on populations built for its paths (``sf.select_population``), lr = 0 and a zero gradient so the
    particles stay put: the distances within D + 2 ulp of the longdouble reference, h_out the median of exactly the doubles read
    back, squared, over log B, to 4 ulp -- a rank off by one among near-ties fails it."""
    x = sf.select_population(kind, B, D)
    z = np.zeros_like(x)
    mu, nu, nm, x_out, h_out, dist = _svgd_step(x, z, z, z, z, 1.0, 1, 0.0)
    assert np.array_equal(x_out, x)  # (mu and nu take the repulsion term; lr = 0 keeps the particles)
    du, hu = _check_distances_and_select(x_out, dist, h_out, B, D, exact=kind == "denormal")
    RECORDS["select"].append({"name": f"{kind} B={B} D={D}", "dist_ulp": du, "h_ulp": hu})
    print(f"sampler fuzz select {kind} B={B} D={D}: distances {du:.2f} ulp, h_out {hu:.2f} ulp (h_out = {h_out!r})")
    assert du <= D + 2 and hu <= 4.0
