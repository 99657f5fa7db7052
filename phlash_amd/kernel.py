"""The kernel plugin: ``get_kernel(M, data, double_precision)`` -> an object with ``.loglik`` and
``.__call__`` -- the drop-in boundary of the reference (src/phlash/kernel.py:7-24; protocol of
``PSMCKernel`` src/phlash/gpu.py:328-438 and ``PureJaxPSMCKernel`` src/phlash/hmm.py:14-49).

What differs from the reference, by design:
* arrays are torch tensors on the GPU (numpy in -> numpy out is kept for the reference's call style);
* ``loglik`` is a ``torch.autograd.Function`` instead of a ``jax.custom_vjp`` (gpu.py:441-472), and
  it is natively batched over particles and chunks instead of being vmapped;
* ``overlap=W`` (extension): rows of ``data`` then carry W leading warm-up sites that are run but
  not scored, so the reference's separate warm-up scan + pi substitution (model.py:52-55) and its
  AD happen inside the same kernel sweep;
* there is **no fallback**: where the reference falls back to pure JAX on ImportError/RuntimeError
  (kernel.py:14-24), this raises -- a silent CPU path would void every parity and speed claim.
"""

from __future__ import annotations

import warnings
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .engine import HipEngine
from .params import PSMCParams
from .size_history import DemographicModel

F64 = torch.float64


def _as_tensor(a, device):
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=F64)
    return torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=F64, device=device)


def _guarded(kern, method: str, *args, **kw):
    """engine.<method> (``run`` or a sweep) with the safety net of the rescale interval: if the forward kernel reports that
    the parameters are too extreme for rescaling every few sites only, switch this kernel object to
    per-site rescaling (the reference's schedule, hmm.py:77-79) for good and evaluate again.
    Rank-local on purpose: ``loglik`` / ``__call__`` contain no collective, so a rank may redo its own
    evaluation without its peers.  The sharded evaluation (``parallel.py``, used by ``fit``) must NOT
    decide locally -- its redo contains an all-reduce -- and carries the flags in that all-reduce
    instead (``take_flags_into`` / ``check_rescaling(collective=True)``).  A chunk index outside
    [0, N) surfaces here as AssertionError (gpu.py:197-199).  Every sweep raises the same underflow flag (path sampling
    also for a draw whose weights have no mass)."""
    out = getattr(kern._eng, method)(*args, **kw)
    if kern._eng.underflow_risk():
        warnings.warn("extreme HMM parameters: switching to per-site rescaling for this kernel object")
        kern._eng.set_rescale_interval(1)
        out = getattr(kern._eng, method)(*args, **kw)
    return out


class PathSample(NamedTuple):
    """What ``PSMCKernel.sample_paths`` returns (device tensors, batch dims stripped as ``loglik`` strips them)."""

    ll: torch.Tensor  # log P(o), float64 (what ``posterior`` returns)
    paths: torch.Tensor  # [..., n_samples, L - overlap] uint8: the sampled states at the scored sites


class TractSample(NamedTuple):
    """What ``PSMCKernel.sample_tracts`` returns (device tensors, batch dims stripped as ``loglik`` strips them)."""

    ll: torch.Tensor  # log P(o), float64 (what ``posterior`` returns)
    counts: torch.Tensor  # [..., n_samples, 4] int32: sites inside the set, tracts, longest tract, changes of state
    hist: torch.Tensor  # [..., n_samples, C] int32: tracts per length class, C = len(edges) + 1
    cover: torch.Tensor | None  # [..., nbin] int32: sites in tracts of at least min_len sites, summed over the samples, or None


class Transitions(NamedTuple):
    """What ``PSMCKernel.transitions`` returns (device tensors, batch dims stripped as ``loglik`` strips them)."""

    ll: torch.Tensor  # log P(o), float64 (what ``posterior`` returns)
    changes: torch.Tensor  # [..., nbin, 2]: bin sums of the expected moves to an older / a younger state
    arrivals: torch.Tensor | None  # [..., nbin, 3, M]: bin means of (stay, up, down) per state, or None


class PairCounts(NamedTuple):
    """What ``PSMCKernel.pair_counts`` returns (device tensors, batch dims stripped as ``loglik`` strips them)."""

    ll: torch.Tensor  # log P(o), float64 (what ``posterior`` returns)
    counts: torch.Tensor  # [..., M, M] float64, origin state first: expected moves from state i to state j over the row's own scored sites


class Predictive(NamedTuple):
    """What ``PSMCKernel.predictive`` returns (device tensors, batch dims stripped as ``loglik`` strips them; the last three are
    views of one track)."""

    ll: torch.Tensor  # log P(o), float64 (what ``posterior`` returns)
    het_observed: torch.Tensor  # [..., nbin]: bin sums of P(o_t = het | o_{-t}) over the observed sites
    het_missing: torch.Tensor  # [..., nbin]: the same over the missing sites
    score: torch.Tensor  # [..., nbin]: bin sums of log P(o_t | o_{-t}) over the observed sites


class Tracts(NamedTuple):
    """What ``PSMCKernel.tracts`` returns (device tensors, batch dims stripped as ``loglik`` strips them)."""

    ll: torch.Tensor  # log P(o), float64 (what ``posterior`` returns)
    prob: torch.Tensor  # [..., nbin]: E[prod of weights(z_t) over the bin's sites | o]


class IntervalTracts(NamedTuple):
    """What ``PSMCKernel.interval_tracts`` returns (float64 device tensors)."""

    ll: torch.Tensor  # log P(o), float64 (what ``posterior`` returns)
    logp: torch.Tensor  # [n] or [B, n], the caller's order: log P(every site of the interval has its state in the set | o)


def _host_ints(x) -> np.ndarray:
    return np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)


def pack_state_masks(masks, n: int, B: int, M: int) -> np.ndarray:
    """State sets as 64-bit words, uint64 [n] or [B, n]: ``masks`` as integers ([n] or [B, n], bit k set = state k is inside; a
    negative int64 is its bit pattern) or as boolean rows ([n, M] or [B, n, M]).  Bits at or above ``M`` are dropped."""
    m = _host_ints(masks)
    assert M <= 64, "a state set is a 64-bit mask"
    if m.dtype == np.bool_:
        assert m.shape in ((n, M), (B, n, M)), f"masks: bool [{n}, {M}] or [{B}, {n}, {M}], got {m.shape}"
        w = (m.astype(np.uint64) << np.arange(M, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    else:
        assert m.shape in ((n,), (B, n)), f"masks: integers [{n}] or [{B}, {n}], got {m.shape}"
        if m.dtype == object:
            w = np.array([int(v) & ((1 << 64) - 1) for v in m.reshape(-1)], dtype=np.uint64).reshape(m.shape)
        elif np.issubdtype(m.dtype, np.signedinteger):
            w = m.astype(np.int64).view(np.uint64)
        else:
            assert np.issubdtype(m.dtype, np.unsignedinteger), f"masks: integers or booleans, got {m.dtype}"
            w = m.astype(np.uint64)
    return w & np.uint64((1 << M) - 1)


def pack_intervals(intervals, own: np.ndarray):
    """``intervals`` = (row, start, end) of n half-open intervals in reported sites, any order; ``own`` [S]: the reported sites of
    every chunk position.  -> (order [n]: the caller's indices sorted by (row, start), iv_off [S + 1], start [n], end [n] in
    that order, max_len).  Raises ValueError, naming the caller's entry, for a row outside [0, S), an empty interval, one out of
    range or beyond the row's own length, and for two intervals of a row that overlap."""
    assert len(intervals) >= 3, "intervals: (row, start, end)"
    row, start, end = (_host_ints(x).astype(np.int64).reshape(-1) for x in intervals[:3])
    n, S = row.shape[0], int(own.shape[0])
    assert start.shape[0] == n and end.shape[0] == n, "intervals: row, start and end of one length"
    order = np.lexsort((start, row))
    r, s, e = row[order], start[order], end[order]

    def first(cond, what):
        if cond.any():
            k = int(np.argmax(cond))
            raise ValueError(f"interval {int(order[k])} (row {int(r[k])}, start {int(s[k])}, end {int(e[k])}): {what}")

    first((r < 0) | (r >= S), f"row outside [0, {S})")
    first(s >= e, "empty: start must be below end")
    first(s < 0, "out of range: start below 0")
    first(e > own[r], "out of range: end beyond the row's own length")
    if n > 1:
        clash = np.concatenate([[False], (r[1:] == r[:-1]) & (s[1:] < e[:-1])])
        first(clash, "overlaps the interval before it in its row")
    off = np.zeros(S + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(r, minlength=S))
    return order, off, s, e, int((e - s).max()) if n else 1


class BinMoments(NamedTuple):
    """What ``PSMCKernel.bin_moments`` returns (float64 device tensors, batch dims stripped as ``loglik`` strips them)."""

    ll: torch.Tensor  # log P(o), float64 (what ``posterior`` returns)
    mean: torch.Tensor  # [..., nbin]: E[sum of values(z_t) over the bin's own sites | o]
    var: torch.Tensor  # [..., nbin]: the posterior variance of that sum
    m1: torch.Tensor  # [..., nbin]: E[S | o] of the centred and scaled row the kernel ran on
    m2: torch.Tensor  # [..., nbin]: E[S^2 | o] of the same row


class LocalRatio(NamedTuple):
    """What ``PSMCKernel.local_ratio`` returns (device tensors, batch dims stripped as ``loglik`` strips them)."""

    ll: torch.Tensor  # log P(o), float64 (what ``posterior`` returns)
    log_ratio: torch.Tensor  # [..., nbin]: log P(o | the bin under the alternative) - log P(o)


class Viterbi(NamedTuple):
    """What ``PSMCKernel.viterbi`` returns (device tensors, batch dims stripped as ``loglik`` strips them)."""

    logp: torch.Tensor  # log probability of the most probable path (z_0 included), float64
    path: torch.Tensor  # [..., L - overlap] uint8: its states at the scored sites; 255 past a row's own length


class Posterior(NamedTuple):
    """What ``PSMCKernel.posterior`` returns (device tensors, batch dims stripped as ``loglik`` strips them)."""

    ll: torch.Tensor  # log P(o), float64
    mean: torch.Tensor | None  # [..., nbin]: bin means of sum_k values_k gamma_t(k), or None without values
    marginals: torch.Tensor | None  # [..., nbin, M]: bin means of gamma_t, or None


class _LogLik(torch.autograd.Function):
    """ll = kernel(params); backward = cotangent * stored d ll / d params (gpu.py:441-472: the fwd
    rule runs the gradient kernel and the bwd rule scales the stored derivative)."""

    @staticmethod
    def forward(ctx, params, kern, inds, need_grad):
        # params [B, S|1, 7, K] float64 on the device
        if need_grad:
            ll, g = _guarded(kern, "run", params, inds, warmup=kern.overlap, grad=True, dlog=False)
            ctx.save_for_backward(g)
            ctx.bcast = params.shape[1] == 1 and inds.shape[0] > 1
        else:
            ll = _guarded(kern, "run", params, inds, warmup=kern.overlap, grad=False)
        return ll

    @staticmethod
    def backward(ctx, gll):
        (g,) = ctx.saved_tensors
        gp = gll[..., None, None] * g.to(F64)
        if ctx.bcast:
            gp = gp.sum(1, keepdim=True)
        return gp, None, None, None


class PSMCKernel:
    """PSMC likelihood kernel on one MI355X.

    Args (reference: gpu.py:328-350):
        M: number of hidden states, 2..64 (compiled sizes 4, 8, 16, 32, 64; others are padded to the
            next one; the reference is tuned for 16).
        data: int8 [N, L] het matrix, values -1 (missing), 0, 1 (larger counts are clipped to 1).
        double_precision: float64 kernels instead of float32.
        num_gpus: accepted for signature compatibility.  One kernel object drives one GPU; scale
            out with one process per GPU (``phlash_amd.parallel``), not with threads.
        overlap: number of leading warm-up sites in every row (extension, default 0).
        device: HIP device ordinal (default: torch's current device).
        keep_host_data: keep a host copy of ``data`` as ``.host_data`` (needed only by the
            reference-style two-step ``log_density(mcp, c, inds, warmup, kern)`` call form,
            model.py:52-57, which concatenates warm-up columns to rows of the kernel's data).
    """

    def __init__(self, M, data, double_precision=False, num_gpus: int = None, overlap: int = 0, device=None,
                 keep_host_data: bool = False):
        if num_gpus is not None:
            assert num_gpus > 0  # gpu.py:340-341
            if num_gpus > 1:
                warnings.warn("num_gpus > 1 is ignored: one PSMCKernel drives one GPU; "
                              "use phlash_amd.parallel (one process per GPU) to scale out")
        if M != 16:
            warnings.warn("Performance is optimized when M=16")  # gpu.py:128-129
        if device is None:
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        if isinstance(data, torch.Tensor):
            if not data.is_cuda:
                data = data.numpy()
        if not isinstance(data, torch.Tensor):
            data = np.asarray(data)
            assert data.ndim == 2  # gpu.py:103
            assert data.dtype == np.int8  # gpu.py:104
            assert data.min() >= -1  # gpu.py:105
            assert np.all(data.max(axis=1) > -1), "data contains observations with all missing values"
        self.M = M
        self.double_precision = double_precision
        self.overlap = int(overlap)
        self.host_data = None
        if keep_host_data:
            self.host_data = data.cpu().numpy() if isinstance(data, torch.Tensor) else np.array(data, copy=True)
        self._flags = None  # [2] float64 on the device: flags of the evaluations since the last check
        self._pinned, self._pin_turn = None, 0  # host slots of begin_check / finish_check
        self._eng = HipEngine(M, data, double_precision=double_precision, device=device)
        self.N, self.L = self._eng.N, self._eng.L
        assert 0 <= self.overlap <= self.L
        self.device = self._eng.device

    @property
    def float_type(self):  # gpu.py:176-180
        return np.float64 if self.double_precision else np.float32

    # ---- shape handling (gpu.py:188-213) ----------------------------------------------------
    def _prepare(self, pp: PSMCParams, index):
        """-> params [B, S|1, 7, M] f64 on device, inds int64 [S] on device, (added_B, added_S)"""
        dev = self.device
        pa = torch.stack([_as_tensor(a, dev) for a in pp], -2)
        if isinstance(index, torch.Tensor):
            inds = index.to(device=dev, dtype=torch.int64)
        else:
            inds = torch.as_tensor(np.asarray(index), dtype=torch.int64, device=dev)
        M = self.M
        added_S = inds.ndim == 0
        inds = torch.atleast_1d(inds)
        assert inds.ndim == 1
        S = inds.shape[0]
        if S > 0:
            lo, hi = int(inds.min()), int(inds.max())
            assert 0 <= lo and hi < self.N, f"0 <= {lo} <= {hi} < N={self.N}"  # gpu.py:197-199
        added_B = False
        if pa.ndim == 2:  # one block for everything
            assert pa.shape == (7, M)
            pa = pa[None, None]
            added_B = True
        elif pa.ndim == 3:  # one block per chunk
            assert pa.shape == (S, 7, M), (pa.shape, S)
            pa = pa[None]
            added_B = True
        assert pa.ndim == 4 and pa.shape[2:] == (7, M)
        assert pa.shape[1] in (1, S)
        assert bool(torch.isfinite(pa).all()), "not all parameters finite"  # gpu.py:214
        return pa, inds, added_B, added_S

    def _model_inputs(self, pp, index):
        """``_prepare`` for a model given as PSMCParams or DemographicModel (convenience overload, gpu.py:364-367)."""
        if isinstance(pp, DemographicModel):
            pp = PSMCParams.from_dm(pp)
        return self._prepare(PSMCParams(*(_as_tensor(a, self.device) for a in pp)), index)

    def _lens_tensor(self, lens):
        """``lens`` ([N] integers, one own length per data row, ``overlap < len <= L``) as int64 on the device, or None."""
        if lens is None:
            return None
        lens = torch.as_tensor(np.asarray(lens.cpu() if isinstance(lens, torch.Tensor) else lens, dtype=np.int64),
                               dtype=torch.int64, device=self.device)
        assert lens.shape == (self.N,), f"lens: one length per data row, [{self.N}]"
        assert int(lens.min()) > self.overlap and int(lens.max()) <= self.L, f"overlap={self.overlap} < lens <= L={self.L}"
        return lens

    @staticmethod
    def _strip(x, added_B, added_S):
        # gpu.py:318-325
        if added_B and added_S:
            return x[0, 0]
        if added_B:
            return x[0]
        if added_S:
            return x[:, 0]
        return x

    # ---- differentiable log-likelihood (gpu.py:359-367) --------------------------------------
    def loglik(self, pp, index):
        """Log-likelihood of chunk(s) ``index`` under ``pp`` (PSMCParams or DemographicModel;
        fields [M], [S, M], [B, S, M], or [B, 1, M] = one block per particle broadcast over the chunks).  Returns a float64 tensor
        of shape (), [S] or [B, S], differentiable w.r.t. the fields of ``pp`` by autograd."""
        pa, inds, added_B, added_S = self._model_inputs(pp, index)
        need_grad = torch.is_grad_enabled() and pa.requires_grad
        ll = _LogLik.apply(pa, self, inds, need_grad)
        return self._strip(ll, added_B, added_S)

    # ---- the raw operator (gpu.py:386-423, 182-325) ------------------------------------------
    def __call__(self, pp: PSMCParams, index, grad: bool):
        """ll (float64) or (ll, PSMCParams of d ll / d log(param)) -- the reference's operator:
        the derivative is with respect to the LOG of each parameter (gpu.py:647-653, 686-691),
        in ``float_type``, batch dims stripped as the reference strips them.  numpy in -> numpy
        out; torch in -> torch out."""
        want_numpy = not any(isinstance(a, torch.Tensor) for a in pp)
        pa, inds, added_B, added_S = self._prepare(pp, index)
        with torch.no_grad():
            if grad:
                ll, g = _guarded(self, "run", pa, inds, warmup=self.overlap, grad=True, dlog=True)
            else:
                ll = _guarded(self, "run", pa, inds, warmup=self.overlap, grad=False)
        ll = self._strip(ll, added_B, added_S)
        if want_numpy:
            ll = ll.cpu().numpy()
        if not grad:
            return ll
        dll = PSMCParams(*(self._strip(g[..., i, :], added_B, added_S) for i in range(7)))
        if want_numpy:
            dll = PSMCParams(*(a.cpu().numpy() for a in dll))
        return ll, dll

    # ---- posterior decoding (psmc -d) ---------------------------------------------------------
    def posterior(self, pp, index, *, values=None, bin: int = 1, marginals: bool = True) -> Posterior:
        """Hidden-state posteriors gamma_t(k) = P(z_t = k | o) of the scored sites (the ``overlap`` warm-up sites are run,
        conditioned on, and not reported) of chunk(s) ``index`` under ``pp`` (PSMCParams or DemographicModel, batch shapes
        as ``loglik``), as means over bins of ``bin`` sites: ``marginals`` [..., nbin, M] and, with ``values`` ([M] or
        [B, M]: a value per state, e.g. ``dm.eta.ect()``), ``mean`` [..., nbin] = bin means of sum_k values_k gamma_t(k).
        nbin = ceil((L - overlap) / bin).  Returns ``Posterior(ll, mean, marginals)``, device tensors in ``float_type``
        (ll float64); no gradient."""
        with torch.no_grad():
            pa, inds, added_B, added_S = self._model_inputs(pp, index)
            vals = None
            if values is not None:
                vals = _as_tensor(values, self.device)
                if vals.ndim == 2 and vals.shape[0] == 1:
                    vals = vals[0]
            ll, m, g = _guarded(self, "posterior", pa, inds, warmup=self.overlap, values=vals, bin=int(bin),
                                          marginals=bool(marginals), mean=vals is not None)
        strip = lambda x: None if x is None else self._strip(x, added_B, added_S)  # noqa: E731
        return Posterior(strip(ll), strip(m), strip(g))

    # ---- transition posteriors ------------------------------------------------------------------
    def transitions(self, pp, index, *, bin: int = 1, lens=None, arrivals: bool = True) -> Transitions:
        """Pair posteriors of adjacent sites, split by how the state at a scored site was reached: ``arrivals``
        [..., nbin, 3, M], the bin means of stay_t(k) = P(z_prev = k, z_t = k | o), up_t(k) = P(z_prev < k, z_t = k | o) and
        down_t(k) = P(z_prev > k, z_t = k | o) (they add up to the marginal ``posterior`` reports), and ``changes``
        [..., nbin, 2], the bin SUMS of sum_k up_t(k) and sum_k down_t(k): the expected number of moves to an older and to a
        younger TMRCA state inside the bin (a change of state, not a recombination event: a recombination that coalesces
        again in the same interval stays).  Chunk(s) ``index`` under ``pp`` (PSMCParams or DemographicModel, batch shapes as
        ``loglik``); bins of ``bin`` scored sites, nbin = ceil((L - overlap) / bin).  ``lens`` ([N] integers, one own length
        per row of the kernel's data, ``overlap < len <= L``): sites at or past a row's own length add nothing and are not
        counted in a mean.  Returns ``Transitions(ll, changes, arrivals)``, device tensors in ``float_type`` (ll float64);
        no gradient."""
        with torch.no_grad():
            pa, inds, added_B, added_S = self._model_inputs(pp, index)
            lens = self._lens_tensor(lens)
            ll, c, a = _guarded(self, "transitions", pa, inds, warmup=self.overlap, bin=int(bin), lens=lens, arrivals=bool(arrivals))
        strip = lambda x: None if x is None else self._strip(x, added_B, added_S)  # noqa: E731
        return Transitions(strip(ll), strip(c), strip(a))

    # ---- pair counts -----------------------------------------------------------------------------
    def pair_counts(self, pp, index, *, lens=None) -> PairCounts:
        """The pair posterior summed along the row: ``counts`` [..., M, M] float64 with counts[i, j] = the sum over the row's own
        scored sites of P(z_prev = i, z_t = j | o), the expected number of moves from TMRCA state i (first index) to state j --
        the matrix ``transitions`` reduces to (stay, up, down) per state reached, and the Baum-Welch transition statistic.  It
        sums to the number of the row's own scored sites; row i held against row i of the model's transition matrix says whether
        the transition structure fits the data.  Chunk(s) ``index`` under ``pp`` (PSMCParams or DemographicModel, batch shapes as
        ``loglik``).  ``lens`` ([N] integers, one own length per row of the kernel's data, ``overlap < len <= L``): sites at or
        past a row's own length add nothing.  Returns ``PairCounts(ll, counts)``, float64 device tensors for either
        ``float_type``; no gradient."""
        with torch.no_grad():
            pa, inds, added_B, added_S = self._model_inputs(pp, index)
            lens = self._lens_tensor(lens)
            ll, c = _guarded(self, "pair_counts", pa, inds, warmup=self.overlap, lens=lens)
        return PairCounts(self._strip(ll, added_B, added_S), self._strip(c, added_B, added_S))

    # ---- leave-one-out predictive -------------------------------------------------------------
    def predictive(self, pp, index, *, bin: int = 1, lens=None) -> Predictive:
        """What the rest of a row says about each of its sites: phet_t = P(o_t = het | o_{-t}), the probability that scored
        site t is het given every other site of the row (and that it is observed at all), as sums over bins of ``bin`` scored
        sites.  ``het_observed`` [..., nbin] sums phet_t over the bin's observed sites -- the expected number of het windows,
        to be held against the observed count -- ``het_missing`` sums it over the missing sites -- the imputed het count under
        the mask -- and ``score`` sums log P(o_t | o_{-t}) over the observed sites, the leave-one-out log score (missing sites
        add 0).  Chunk(s) ``index`` under ``pp`` (PSMCParams or DemographicModel, batch shapes as ``loglik``); nbin =
        ceil((L - overlap) / bin).  ``lens`` ([N] integers, one own length per row of the kernel's data, ``overlap < len <=
        L``): sites at or past a row's own length add nothing.  Returns ``Predictive(ll, het_observed, het_missing, score)``,
        device tensors in ``float_type`` (ll float64); no gradient."""
        with torch.no_grad():
            pa, inds, added_B, added_S = self._model_inputs(pp, index)
            lens = self._lens_tensor(lens)
            ll, track = _guarded(self, "predictive", pa, inds, warmup=self.overlap, bin=int(bin), lens=lens)
        track = self._strip(track, added_B, added_S)
        return Predictive(self._strip(ll, added_B, added_S), track[..., 0], track[..., 1], track[..., 2])

    # ---- tract posteriors -----------------------------------------------------------------------
    def tracts(self, pp, index, *, weights, bin: int = 1, lens=None) -> Tracts:
        """Where the tracts are: for every bin of ``bin`` scored sites, ``prob`` = E[prod over the bin's sites of
        weights(z_t) | o].  With ``weights`` the indicator of a set of states this is the posterior probability that EVERY site of
        the bin has its state in the set -- a joint event of the bin's sites, exact, which neither the per-site marginals (their
        bin mean is only an upper bound) nor sampled paths (an estimate) give.  ``weights``: [M], or [B, M] with one row per
        particle of ``pp``, values in [0, 1].  Chunk(s) ``index`` under ``pp`` (PSMCParams or DemographicModel, batch shapes as
        ``loglik``); nbin = ceil((L - overlap) / bin).  ``lens`` ([N] integers, one own length per row of the kernel's data,
        ``overlap < len <= L``): a site at or past a row's own length restricts nothing, and a bin without a site of the row's
        own is 0.  Returns ``Tracts(ll, prob)``, device tensors in ``float_type`` (ll float64); no gradient."""
        with torch.no_grad():
            pa, inds, added_B, added_S = self._model_inputs(pp, index)
            w = torch.as_tensor(np.array(weights.cpu() if isinstance(weights, torch.Tensor) else weights, dtype=np.float64),
                                dtype=torch.float64, device=self.device)
            assert w.shape in ((self.M,), (pa.shape[0], self.M)), f"weights: [{self.M}] or [{pa.shape[0]}, {self.M}], got {tuple(w.shape)}"
            assert bool(((w >= 0) & (w <= 1)).all()), "weights must lie in [0, 1]"
            lens = self._lens_tensor(lens)
            ll, tract = _guarded(self, "tracts", pa, inds, w, warmup=self.overlap, bin=int(bin), lens=lens)
        return Tracts(self._strip(ll, added_B, added_S), self._strip(tract, added_B, added_S))

    # ---- interval tracts -----------------------------------------------------------------------
    def interval_tracts(self, pp, index, *, intervals, masks, lens=None) -> IntervalTracts:
        """How sure the data are of a called segment: for each of n intervals with arbitrary ends and a state set of its own,
        ``logp`` = log P(EVERY site of the interval has its state in the set | o) -- ``tracts`` without its fixed grid and its
        single set per call, and as a log with an exponent of its own, so a tract of thousands of sites far below the float range
        is right.  ``intervals`` = (row, start, end): integer arrays or tensors as ``phlash_amd.tmrca_segments`` returns them
        (further entries are ignored); ``row`` is the position in ``index``, ``start`` / ``end`` count scored sites as
        ``viterbi``'s path does (half-open).  The intervals of one row must not overlap; any order.  ``masks``: the sets, as
        integers [n] or [B, n] (bit k set = state k is inside) or as boolean rows [n, M] or [B, n, M]; a leading B gives every
        particle of ``pp`` its own sets.  Chunk(s) ``index`` under ``pp`` (PSMCParams or DemographicModel, batch shapes as
        ``loglik``).  ``lens`` ([N] integers, one own length per row of the kernel's data, ``overlap < len <= L``) bounds each
        row's intervals.  A missing site is restricted to the set like any other.  A full set gives exactly 0, an empty one -inf.
        Raises ValueError for an empty interval, one out of range or beyond ``lens``, and for overlapping intervals.  Returns
        ``IntervalTracts(ll, logp)``, float64 device tensors, ``logp`` [n] or [B, n] in the caller's order; no gradient."""
        with torch.no_grad():
            pa, inds, added_B, added_S = self._model_inputs(pp, index)
            B, S = pa.shape[0], inds.shape[0]
            lens = self._lens_tensor(lens)
            own = (lens[inds].cpu().numpy() if lens is not None else np.full(S, self.L, dtype=np.int64)) - self.overlap
            order, off, start, end, max_len = pack_intervals(intervals, own)
            n = order.shape[0]
            words = pack_state_masks(masks, n, B, self.M)[..., order]
            dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int64, device=self.device)  # noqa: E731
            ll, sorted_logp = _guarded(self, "interval_tracts", pa, inds, dev(off), dev(start), dev(end), dev(words.view(np.int64)),
                                       warmup=self.overlap, max_len=max_len, lens=lens)
            logp = torch.empty_like(sorted_logp)
            logp[:, torch.as_tensor(order, device=sorted_logp.device)] = sorted_logp
        return IntervalTracts(self._strip(ll, added_B, added_S), logp[0] if added_B else logp)

    # ---- bin moments ----------------------------------------------------------------------------
    def bin_moments(self, pp, index, *, values, bin: int = 1, lens=None) -> BinMoments:
        """An error bar for a bin: the posterior mean and variance of S = the sum of ``values``(z_t) over the bin's sites, for
        every bin of ``bin`` scored sites.  The variance is exact and holds the covariances between the bin's sites, which
        dominate it: the per-site marginals give the mean only, and sampled paths only estimate the variance.  With ``values``
        the states' expected coalescence times S / n is the bin's mean TMRCA and sqrt(var) / n its posterior standard deviation;
        with an indicator of a set of states S is how many of the bin's sites have their state in the set.

        ``values``: [M], or [B, M] with one row per particle of ``pp``, any real numbers.  Each particle's row is centred and
        scaled before it goes to the kernel -- c_b = the mean of the row under the particle's own pi (for blocks per chunk: under
        the sum of their pi rows), s_b = max |v - c_b|, the kernel runs on (v - c_b) / s_b in [-1, 1] (zeros where s_b = 0) -- and
        the moments are mapped back in float64: ``mean`` = s m1 + c n and ``var`` = s^2 max(m2 - m1^2, 0), n the number of the
        bin's own sites.  The variance does not depend on the centre, and m2 - m1^2 of a row far from its centre cancels digits
        the float32 recursion does not have.  ``m1`` and ``m2`` are the raw moments of the row the kernel ran on.

        Chunk(s) ``index`` under ``pp`` (PSMCParams or DemographicModel, batch shapes as ``loglik``); nbin =
        ceil((L - overlap) / bin).  ``lens`` ([N] integers, one own length per row of the kernel's data, ``overlap < len <= L``):
        a site at or past a row's own length adds nothing, and a bin without a site of the row's own is 0.  Returns
        ``BinMoments(ll, mean, var, m1, m2)``, float64 device tensors for either ``float_type``; no gradient."""
        with torch.no_grad():
            pa, inds, added_B, added_S = self._model_inputs(pp, index)
            B, S = pa.shape[0], inds.shape[0]
            v = torch.as_tensor(np.array(values.cpu() if isinstance(values, torch.Tensor) else values, dtype=np.float64),
                                dtype=torch.float64, device=self.device)
            assert v.shape in ((self.M,), (B, self.M)), f"values: [{self.M}] or [{B}, {self.M}], got {tuple(v.shape)}"
            assert bool(torch.isfinite(v).all()), "not all values finite"
            v = v.expand(B, self.M)
            # the centre as lo + (mean of v - lo): a row that is constant over the states is its own centre, exactly
            pi = pa[:, :, 6, :].sum(1)  # [B, M]
            lo = v.min(-1, keepdim=True).values
            c = lo + ((v - lo) * pi).sum(-1, keepdim=True) / pi.sum(-1, keepdim=True)
            s = (v - c).abs().max(-1, keepdim=True).values
            vn = torch.where(s > 0, (v - c) / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(v)).clamp_(-1.0, 1.0).contiguous()
            lens = self._lens_tensor(lens)
            ll, m1, m2 = _guarded(self, "bin_moments", pa, inds, vn, warmup=self.overlap, bin=int(bin), lens=lens)
            # the bin's own sites, counted from lens
            own = (lens[inds] if lens is not None else torch.full((S,), self.L, dtype=torch.int64, device=self.device)) - self.overlap
            start = torch.arange(m1.shape[-1], dtype=torch.int64, device=self.device) * int(bin)
            n = (own[:, None] - start[None, :]).clamp_(0, int(bin)).to(torch.float64)  # [S, nbin]
            mean = s[:, :, None] * m1 + c[:, :, None] * n[None]
            var = s[:, :, None] ** 2 * (m2 - m1 * m1).clamp_(min=0.0)
        strip = lambda x: self._strip(x, added_B, added_S)  # noqa: E731
        return BinMoments(strip(ll), strip(mean), strip(var), strip(m1), strip(m2))

    # ---- local likelihood-ratio scans ------------------------------------------------------------
    def local_ratio(self, pp, alt, index, *, bin: int = 1, lens=None) -> LocalRatio:
        """Where the fitted model is wrong, and in which direction: for every bin of ``bin`` scored sites, ``log_ratio`` =
        log P(o | the bin's sites generated by ``alt``, the rest of the row by ``pp``) - log P(o | ``pp``).  Every site of the bin
        has the transition into it and its emission taken from ``alt``; the forward and backward vectors around the bin are those
        of ``pp``, and ``alt``'s pi is never used.  The value is exact and is computed with an exponent of its own, so it is right
        wherever it is representable as a log (the linear ratio need not be).  Special cases: an ``alt`` equal to ``pp`` with
        both emission rows set to 1 gives the block-out predictive, ``log_ratio`` = -log P(o_bin | o_-bin) (at ``bin`` = 1 minus
        the leave-one-out score ``predictive`` reports at the observed sites); an ``alt`` equal to ``pp`` with both emission rows
        multiplied by an indicator of a set of states gives the log of ``tracts``' probability on rows without missing windows
        (a missing window has emission 1 in both models, so there the indicator restricts nothing).  ``alt``: PSMCParams or
        DemographicModel with the batch shapes of ``pp`` or broadcastable to them ([M]: one alternative for everything).
        Chunk(s) ``index`` under ``pp`` (PSMCParams or DemographicModel, batch shapes as ``loglik``); nbin =
        ceil((L - overlap) / bin).  ``lens`` ([N] integers, one own length per row of the kernel's data, ``overlap < len <=
        L``): a site at or past a row's own length is stepped with ``pp``, and a bin without a site of the row's own is 0.
        Returns ``LocalRatio(ll, log_ratio)``, device tensors in ``float_type`` (ll float64); no gradient."""
        if isinstance(alt, DemographicModel):
            alt = PSMCParams.from_dm(alt)
        with torch.no_grad():
            pa, inds, added_B, added_S = self._model_inputs(pp, index)
            B, S, M = pa.shape[0], inds.shape[0], self.M
            al = torch.stack([_as_tensor(a, self.device) for a in alt], -2)
            assert al.shape[-2:] == (7, M) and 2 <= al.ndim <= 4, f"alt: fields [..., {M}], got {tuple(al.shape)}"
            assert bool(torch.isfinite(al).all()), "not all parameters of alt finite"
            if al.ndim == 2:  # one block for everything
                al = al[None, None]
            elif al.ndim == 3:  # one block per chunk, as pp
                al = al[None]
            assert al.shape[0] in (1, B) and al.shape[1] in (1, S), f"alt: batch shape of pp or broadcast to it, got {tuple(al.shape)}"
            lens = self._lens_tensor(lens)
            ll, lr = _guarded(self, "local_ratio", pa, al, inds, warmup=self.overlap, bin=int(bin), lens=lens)
        return LocalRatio(self._strip(ll, added_B, added_S), self._strip(lr, added_B, added_S))

    # ---- Viterbi decoding ---------------------------------------------------------------------
    def viterbi(self, pp, index, *, lens=None) -> Viterbi:
        """The single most probable hidden path (max-product) of chunk(s) ``index`` under ``pp`` (PSMCParams or
        DemographicModel, batch shapes as ``loglik``): ``Viterbi(logp, path)`` with ``path`` [..., L - overlap] uint8, the
        states at the scored sites (the ``overlap`` warm-up sites take part in the maximisation and are not reported), and
        ``logp`` the log probability of the whole path.  ``lens`` ([N] integers, one own length per row of the kernel's data,
        ``overlap < len <= L``): rows end at their own length -- which is not the same as padding them with missing windows
        -- and ``path`` holds 255 past it.  Ties go to the lowest state index.  No gradient."""
        with torch.no_grad():
            pa, inds, added_B, added_S = self._model_inputs(pp, index)
            lens = self._lens_tensor(lens)
            logp, path = _guarded(self, "viterbi", pa, inds, warmup=self.overlap, lens=lens)
        return Viterbi(self._strip(logp, added_B, added_S), self._strip(path, added_B, added_S))

    # ---- posterior path sampling ---------------------------------------------------------------
    def sample_paths(self, pp, index, *, n_samples: int = 1, seed: int = 0) -> PathSample:
        """``n_samples`` whole hidden paths drawn from the posterior, z ~ P(z | o), of chunk(s) ``index`` under ``pp`` (PSMCParams
        or DemographicModel, batch shapes as ``loglik``): ``PathSample(ll, paths)`` with ``paths`` [..., n_samples, L - overlap]
        uint8, the states at the scored sites (the ``overlap`` warm-up sites condition the draws and are not reported).
        Forward filtering, backward sampling; the uniforms come from a counter-based generator keyed by ``seed``: draw r of a
        sequence depends on (seed, the sequence's position in the call, r, site) only, not on ``n_samples``.  No gradient."""
        with torch.no_grad():
            pa, inds, added_B, added_S = self._model_inputs(pp, index)
            ll, paths = _guarded(self, "sample_paths", pa, inds, warmup=self.overlap, n_samples=int(n_samples), seed=int(seed))
        return PathSample(self._strip(ll, added_B, added_S), self._strip(paths, added_B, added_S))

    # ---- sampled tract spectra -------------------------------------------------------------------
    def sample_tracts(self, pp, index, *, in_set, n_samples: int = 1, seed: int = 0, edges=(), lens=None, min_len: int = 1,
                      bin: int | None = None) -> TractSample:
        """What is not additive over sites, from sampled paths that are never stored: the paths ``sample_paths`` draws for the same
        ``seed`` (draw for draw), reduced inside the kernel to their tracts -- maximal runs of consecutive scored sites whose
        state lies in ``in_set`` (bool [M], or [B, M] with one row per particle of ``pp``).  Per sample ``counts``
        [..., n_samples, 4] = (sites inside the set, number of tracts, longest tract, changes of state between adjacent scored
        sites) and ``hist`` [..., n_samples, C], the tracts by length class: ``edges`` (up to 15 strictly ascending lengths >= 1)
        cut the lengths into C = len(edges) + 1 classes, a length equal to an edge going to the upper one.  With ``bin`` given,
        ``cover`` [..., nbin] (nbin = ceil((L - overlap) / bin)): per bin of ``bin`` scored sites, the number of the bin's own
        sites that lie in a tract of at least ``min_len`` sites, summed over the samples -- divided by n_samples x the bin's own
        sites, the estimated probability that a window lies in such a tract.  ``lens`` ([N] integers, one own length per row of
        the kernel's data, ``overlap < len <= L``): sites at or past a row's own length are drawn and count for nothing.  A
        tract that touches the first scored site or the row's last own site is counted at its visible length.  Chunk(s)
        ``index`` under ``pp`` (PSMCParams or DemographicModel, batch shapes as ``loglik``).  ``phlash_amd.path_tracts`` computes
        the same arrays from stored paths.  Returns ``TractSample(ll, counts, hist, cover)``, int32 device tensors (ll float64);
        no gradient."""
        with torch.no_grad():
            pa, inds, added_B, added_S = self._model_inputs(pp, index)
            m = np.asarray(in_set.cpu() if isinstance(in_set, torch.Tensor) else in_set).astype(bool)
            assert m.shape in ((self.M,), (pa.shape[0], self.M)), f"in_set: [{self.M}] or [{pa.shape[0]}, {self.M}], got {m.shape}"
            words = [sum(1 << k for k in range(self.M) if row[k]) for row in m.reshape(-1, self.M)]
            masks = torch.tensor([w - (1 << 64) if w >= 1 << 63 else w for w in words], dtype=torch.int64, device=self.device)
            lens = self._lens_tensor(lens)
            ll, stats, cover = _guarded(self, "sample_tracts", pa, inds, masks, warmup=self.overlap, n_samples=int(n_samples),
                                        seed=int(seed), edges=tuple(int(e) for e in edges), lens=lens, min_len=int(min_len),
                                        bin=None if bin is None else int(bin))
        strip = lambda x: None if x is None else self._strip(x, added_B, added_S)  # noqa: E731
        return TractSample(strip(ll), strip(stats[..., :4]), strip(stats[..., 4:]), strip(cover))

    # ---- fused evaluation used by the sampler -------------------------------------------------
    def _inds_tensor(self, inds) -> torch.Tensor:
        if isinstance(inds, torch.Tensor):  # device-resident indices are range-checked on the device
            return inds.to(device=self.device, dtype=torch.int64)
        a = np.atleast_1d(np.asarray(inds, dtype=np.int64))
        if a.size:  # host indices: the reference's assert (gpu.py:197-199), free here
            assert 0 <= a.min() and a.max() < self.N, f"0 <= {a.min()} <= {a.max()} < N={self.N}"
        return torch.as_tensor(a, dtype=torch.int64, device=self.device)

    def value_and_grad(self, pp: PSMCParams, inds, reduce_chunks: bool = True):
        """One particle population against a minibatch: pp fields [B, M] -> (ll, d ll / d params).
        With ``reduce_chunks`` the sum over the S chunks is taken here (ll [B], grad [B, 7, M]
        float64) -- the quantity model.log_density needs (model.py:57 ``.sum()``).  Asynchronous: no
        host synchronisation, hence no underflow / index check here: the flags stay on the device until
        ``take_flags_into`` (inside the sharded evaluation) or ``check_rescaling`` collects them; ``fit``
        does that once per iteration, where it synchronises anyway."""
        pa = torch.stack([_as_tensor(a, self.device) for a in pp], -2)[:, None]
        with torch.no_grad():
            ll, g = self._eng.run(pa, self._inds_tensor(inds), warmup=self.overlap, grad=True, dlog=False)
        if reduce_chunks:
            return ll.sum(1), g.sum(1, dtype=F64)
        return ll, g

    def value(self, pp: PSMCParams, inds, reduce_chunks: bool = True):
        """The same without the gradient: the no-gradient kernel only (no checkpoint store, no
        backward sweep) -- what the reference's primal rule runs (gpu.py:446-449), e.g. for the ELPD
        of held-out data (mcmc.py:224-238)."""
        pa = torch.stack([_as_tensor(a, self.device) for a in pp], -2)[:, None]
        with torch.no_grad():
            ll = self._eng.run(pa, self._inds_tensor(inds), warmup=self.overlap, grad=False)
        return ll.sum(1) if reduce_chunks else ll

    def take_flags_into(self, dst: torch.Tensor):
        """Stream-ordered (no host sync): move this kernel object's flags (underflow risk, bad chunk
        index) into ``dst`` ([2] float64 on the device, e.g. a slice of the buffer about to be
        all-reduced) and remember ``dst`` as the place ``check_rescaling(collective=True)`` reads."""
        self._eng.take_flags_async(dst)
        self._flags = dst

    def flags_consumed(self):
        """The flags a sharded evaluation moved off the device word (``take_flags_into``) have been read and judged by the
        caller itself (``fit``'s speculative held-out score reads them out of its own all-reduced buffer): forget the buffer,
        so that the next ``check_rescaling`` does not read it a second time."""
        self._flags = None

    def check_rescaling(self, collective: bool = False, also: torch.Tensor | None = None) -> bool:
        """True (after switching to per-site rescaling) if an evaluation since the last check hit
        parameters too extreme for the current rescale interval; the caller should redo that step.
        ``collective``: decide from the flags that travelled in the last all-reduce
        (``take_flags_into``), which are the same on every rank, so that all ranks take the same
        branch -- a rank-local decision followed by a redo that contains a collective would desynchronise
        the ranks.  ``also``: a one-element device tensor the caller wants on the host as well; it travels
        in the same device-to-host copy (one synchronisation instead of two) and is left in
        ``self.also_value`` (float).  Raises AssertionError if a chunk index was out of range (gpu.py:197-199)."""
        self.also_value = None
        if collective and self._flags is None:
            # nothing travelled in an all-reduce since the last check: deciding from the local device word
            # here would be exactly the rank-local decision this mode exists to rule out
            raise RuntimeError("check_rescaling(collective=True) without a preceding sharded evaluation "
                               "(parallel.sharded_loglik_sum / take_flags_into): no reduced flags to read")
        under = bad = 0.0
        if self._flags is not None:
            # flags that a sharded evaluation moved off the device word (take_flags_async clears it there):
            # they count for a plain check as well, or an underflow seen by that evaluation would be lost
            if also is not None:
                both = torch.cat([self._flags.reshape(2), also.reshape(1).to(self._flags.dtype)]).cpu()  # synchronises
                under, bad, self.also_value = (float(v) for v in both)
            else:
                under, bad = (float(v) for v in self._flags.cpu())  # synchronises
            self._flags = None
        elif also is not None:
            self.also_value = float(also)
        _lib.check_failure_slot(bad, f"N={self.N}")
        risk = under > 0
        if not collective:
            risk = self._eng.underflow_risk() or risk  # evaluations that did not go through take_flags_into
        if risk:
            warnings.warn("extreme HMM parameters: switching to per-site rescaling for this kernel object")
            self._eng.set_rescale_interval(1)
            return True
        return False


    def switch_to_per_site_rescaling(self):
        """What a positive underflow flag asks for (the reference's schedule, always safe), for callers that read the
        reduced flags themselves."""
        warnings.warn("extreme HMM parameters: switching to per-site rescaling for this kernel object")
        self._eng.set_rescale_interval(1)

    def begin_check(self, also: torch.Tensor):
        """First half of ``check_rescaling(collective=True, also=...)``: queues the copy of the reduced flags and of
        ``also`` to pinned host memory on the current stream and returns at once, so that the caller can launch its
        next step before it looks at this one's flags (phlash_amd.mcmc.fit does).  ``finish_check`` is the other half."""
        if self._flags is None:
            raise RuntimeError("begin_check without a preceding sharded evaluation (parallel.sharded_loglik_sum / "
                               "take_flags_into): no reduced flags to read")
        dev = torch.cat([self._flags.reshape(2), also.reshape(1).to(self._flags.dtype)])
        self._flags = None
        if self._pinned is None:  # two slots: a caller holds at most one check open while it begins the next
            self._pinned = [torch.empty(3, dtype=F64).pin_memory() for _ in range(2)]
        self._pin_turn ^= 1
        slot = self._pinned[self._pin_turn]
        slot.copy_(dev, non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.device))
        return slot, done

    def finish_check(self, pending) -> bool:
        """Second half: waits for the copy ``begin_check`` queued, then decides like ``check_rescaling`` (True = the
        step those flags belong to has to be redone, per-site rescaling is switched on; ``also_value`` is set)."""
        slot, done = pending
        done.synchronize()
        under, bad, self.also_value = (float(v) for v in slot)
        _lib.check_failure_slot(bad, f"N={self.N}")
        if under > 0:
            warnings.warn("extreme HMM parameters: switching to per-site rescaling for this kernel object")
            self._eng.set_rescale_interval(1)
            return True
        return False


def get_kernel(M: int, data, double_precision: bool = False, **kw) -> PSMCKernel:
    """Reference signature (src/phlash/kernel.py:7).  Raises if the HIP library or a GPU is
    missing -- there is deliberately no slower fallback to hide behind."""
    return PSMCKernel(M=M, data=data, double_precision=double_precision, **kw)
