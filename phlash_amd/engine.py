"""Thin device-side wrapper around one ``phk_handle``: torch tensors in, torch tensors out.

This is the layer the reference has in ``_PSMCKernelBase`` (src/phlash/gpu.py:101-325), minus the
per-call host<->device traffic: parameters, indices, log-likelihoods and gradients are torch tensors
on the handle's GPU, passed to the C ABI by pointer.  PyTorch is plumbing here (device memory and
streams); all arithmetic on the path happens in the HIP kernels.
"""

from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _lib


COMPILED_K = (4, 8, 16, 32, 64)


class _SweepCall(NamedTuple):
    """The arguments the sweeps' C entry points share (``HipEngine._sweep_call``)."""

    head: tuple  # handle, params, pstride_b, pstride_s, prefold
    grid: tuple  # inds, B, S
    B: int
    S: int
    pad_k: int  # padding states beyond the caller's K
    lens: int | None  # device pointer
    stream: ctypes.c_void_p
    keep: tuple  # the tensors behind the pointers: alive until the call is enqueued


class HipEngine:
    """K hidden states.  The kernels are compiled for K in {4, 8, 16, 32, 64}; any other K <= 64 runs
    on the next compiled size with unreachable padding states (zero transition / initial mass,
    emission 1), which changes nothing: their alpha stays exactly 0."""

    def __init__(self, K: int, data, double_precision: bool = False, device: int = 0):
        lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: phlash_amd needs an MI355X (there is no CPU fallback)")
        self.K_user = int(K)
        if not 2 <= self.K_user <= COMPILED_K[-1]:
            raise NotImplementedError(f"K={K} outside [2, {COMPILED_K[-1]}]")
        K = min(k for k in COMPILED_K if k >= self.K_user)
        self.K = int(K)
        self.double_precision = bool(double_precision)
        self.device = torch.device("cuda", int(device))
        self.dtype = torch.float64 if double_precision else torch.float32
        # float64 parameter blocks handed to a float32 kernel object are rounded together with their folded factors
        # (``run``); False = round the rows only and let the kernels fold them, as a caller with float32 blocks gets it
        self.prefold = True
        # ... and a gradient call's ll is corrected to first order for what the rounding did to the model (phk_ll_first_order)
        self.first_order = True
        self._h = ctypes.c_void_p()
        if isinstance(data, torch.Tensor) and data.is_cuda:
            # device-resident matrix: validate with torch (gpu.py:103-113), hand over the pointer
            assert data.ndim == 2 and data.dtype == torch.int8
            assert int(data.min()) >= -1
            assert bool((data.max(dim=1).values > -1).all()), "data contains observations with all missing values"
            d = data.contiguous()
            self.N, self.L = d.shape
            rc = lib.phk_create(ctypes.byref(self._h), self.K, d.data_ptr(), self.N, self.L, 1, int(double_precision), int(device))
        else:
            d = np.asarray(data)
            assert d.ndim == 2  # gpu.py:103
            assert d.dtype == np.int8  # gpu.py:104
            d = np.ascontiguousarray(d)
            self.N, self.L = d.shape
            rc = lib.phk_create(ctypes.byref(self._h), self.K, d.ctypes.data, self.N, self.L, 0, int(double_precision), int(device))
        _lib.check(rc)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.load().phk_destroy(h)

    def __del__(self):  # gpu.py:153-174
        try:
            self.close()
        except Exception:
            pass

    # ---- tuning / introspection -----------------------------------------------------------
    def set_variant(self, R: int = 0, T: int = 0):
        _lib.check(_lib.load().phk_set_variant(self._h, int(R), int(T)))

    def set_rescale_interval(self, nrm: int = 0):
        _lib.check(_lib.load().phk_set_rescale_interval(self._h, int(nrm)))
        self._nrm = int(nrm)

    def underflow_risk(self) -> bool:
        """True if a call since the last query ran into parameters too extreme for rescaling only
        every few sites (synchronises).  The caller should re-evaluate with set_rescale_interval(1)."""
        f = ctypes.c_int()
        _lib.check(_lib.load().phk_underflow_risk(self._h, ctypes.byref(f)))
        return bool(f.value)

    def take_flags_async(self, dst: torch.Tensor):
        """Stream-ordered, no host synchronisation: dst[0] = 1.0 on underflow risk, dst[1] = 1.0 if a
        chunk index was out of range (``dst``: two contiguous float64 on the device); clears the flags."""
        assert dst.is_cuda and dst.dtype == torch.float64 and dst.numel() == 2 and dst.is_contiguous()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(_lib.load().phk_take_flags_async(self._h, dst.data_ptr(), ctypes.c_void_p(stream)))

    def reduce_chunks(self, ll: torch.Tensor, g: torch.Tensor, buf: torch.Tensor):
        """Outputs of ``run`` (ll [B, S] float64, g [B, S, 7, K] in the handle's float type) -> ``buf`` [B + 1, 1 + 7K]
        float64: row b = [sum_s ll, sum_s g]; row B = this handle's flags as by ``take_flags_async`` (the device word
        is cleared).  One launch, stream-ordered (``phk_reduce_chunks``)."""
        B, S = ll.shape
        assert g.is_contiguous() and ll.is_contiguous() and g.shape == (B, S, 7, self.K) and g.dtype == self.dtype
        assert buf.is_contiguous() and buf.dtype == torch.float64 and buf.shape == (B + 1, 1 + 7 * self.K)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(_lib.load().phk_reduce_chunks(self._h, ll.data_ptr(), g.data_ptr(), B, S, buf.data_ptr(), ctypes.c_void_p(stream)))

    def set_loop_budget_scale(self, kernels: int = 7, num: int = 1, den: int = 1):
        """Test hook (``phk_set_loop_budget_scale``): scale the iteration budgets of the forward kernel (bit 0), the backward
        kernel (bit 1), the beta scan (bit 2)."""
        _lib.check(_lib.load().phk_set_loop_budget_scale(self._h, int(kernels), int(num), int(den)))

    def block_rescale_counts(self) -> tuple[np.ndarray, int]:
        """Test hook (``phk_block_rescale_counts``, synchronises): per sequence of the last gradient call's last launch, the
        number of checkpoint blocks in which the forward kernel took a power of two out of the state, and the blocks per
        sequence."""
        b, c = self.get_slab()
        counts = np.zeros(max(b * c, 1), dtype=np.int64)
        blocks = ctypes.c_int64()
        _lib.check(_lib.load().phk_block_rescale_counts(self._h, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                        counts.size, ctypes.byref(blocks)))
        return counts[: b * c], blocks.value

    def set_asm_run(self, on: bool):
        """The hand-written block-run sequence of the K = 16 float32 sweeps on / off (``phk_set_asm_run``; off = the C++ body)."""
        _lib.check(_lib.load().phk_set_asm_run(self._h, int(bool(on))))

    def set_fwd_run(self, on: bool):
        """The hand-written run of lean pieces of the K = 16 float32 forward kernel on / off (``phk_set_fwd_run``; off = the C++ body)."""
        _lib.check(_lib.load().phk_set_fwd_run(self._h, int(bool(on))))

    def get_fwd_run(self) -> bool:
        """Whether the forward kernel of this handle uses that sequence (``phk_get_fwd_run``)."""
        return bool(_lib.load().phk_get_fwd_run(self._h))

    def get_asm_run(self) -> bool:
        """Whether the sweeps of this handle use that sequence: the default for K = 16 float32 (``phk_get_asm_run``)."""
        return bool(_lib.load().phk_get_asm_run(self._h))

    def set_deterministic(self, on: bool):
        _lib.check(_lib.load().phk_set_deterministic(self._h, int(bool(on))))

    def set_autotune(self, on: bool):
        _lib.check(_lib.load().phk_set_autotune(self._h, int(bool(on))))

    def set_backward_mode(self, mode: int = -1):
        """-1 automatic, 0 serial sweep per sequence, 1 segmented (small batches)."""
        _lib.check(_lib.load().phk_set_backward_mode(self._h, int(mode)))

    def set_plan(self, segmented: int = -1, R: int = 0, T: int = 8, R_forward: int = 0, R_scan: int = 0):
        _lib.check(_lib.load().phk_set_plan(self._h, int(segmented), int(R), int(T), int(R_forward), int(R_scan)))

    def install_plan(self, plan: dict):
        """Force exactly the plan another handle's ``get_plan`` reported (e.g. rank 0's tuned plan on every rank)."""
        if plan["segmented"]:
            self.set_plan(1, plan["R"], plan["T"], plan["R_forward"], plan["R_scan"])
            return
        self.set_plan(0, plan["R"], plan["T"], plan["R_forward"], 0)
        _lib.check(_lib.load().phk_set_plan_hybrid(self._h, int(plan.get("hybrid_first", 0)),
                                                   int(plan.get("R_segment_sweep", 0)), int(plan.get("R_scan", 0))))

    def get_plan(self) -> dict:
        v = [ctypes.c_int() for _ in range(5)]
        _lib.check(_lib.load().phk_get_plan(self._h, *(ctypes.byref(x) for x in v)))
        plan = dict(zip(("segmented", "R", "T", "R_forward", "R_scan"), (x.value for x in v)))
        first, r3, r2 = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
        _lib.check(_lib.load().phk_get_plan_hybrid(self._h, ctypes.byref(first), ctypes.byref(r3), ctypes.byref(r2)))
        if first.value > 0:  # serial sweep of the first `hybrid_first` sequences || segment sweep of the rest
            plan.update(hybrid_first=first.value, R_segment_sweep=r3.value, R_scan=r2.value)
        return plan

    def get_variant(self, B: int, S: int) -> tuple[int, int]:
        r, t = ctypes.c_int(), ctypes.c_int()
        _lib.check(_lib.load().phk_get_variant(self._h, int(B), int(S), ctypes.byref(r), ctypes.byref(t)))
        return r.value, t.value

    def set_workspace_limit(self, nbytes: int):
        _lib.check(_lib.load().phk_set_workspace_limit(self._h, int(nbytes)))

    def workspace_bytes(self) -> int:
        return int(_lib.load().phk_workspace_bytes(self._h))

    def get_slab(self) -> tuple[int, int]:
        """(particles, chunks) per launch of the last call (the checkpoint store is cut into slabs
        when it would exceed the workspace limit)."""
        b, c = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(_lib.load().phk_get_slab(self._h, ctypes.byref(b), ctypes.byref(c)))
        return b.value, c.value

    def set_profiling(self, on: bool):
        _lib.check(_lib.load().phk_set_profiling(self._h, int(bool(on))))

    def last_timing(self) -> tuple[float, float, int]:
        f, b, n = ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
        _lib.check(_lib.load().phk_last_timing(self._h, ctypes.byref(f), ctypes.byref(b), ctypes.byref(n)))
        return f.value, b.value, n.value

    def timing_totals(self) -> tuple[float, float, int]:
        """(forward ms, backward ms, launches) summed over all calls since the last query."""
        f, b, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        _lib.check(_lib.load().phk_timing_totals(self._h, ctypes.byref(f), ctypes.byref(b), ctypes.byref(n)))
        return f.value, b.value, n.value

    # ---- the operator -----------------------------------------------------------------------
    def _pad_states(self, blocks: torch.Tensor) -> torch.Tensor:
        """Parameter blocks [.., .., 7, K_user] padded to the compiled size: rows b, d, u, v, pi with 0, emission rows with 1."""
        if self.K_user == self.K:
            return blocks
        pad = torch.zeros(blocks.shape[:3] + (self.K - self.K_user,), dtype=blocks.dtype, device=blocks.device)
        pad[:, :, 4:6, :] = 1.0
        return torch.cat([blocks, pad], -1)

    def _blocks(self, x: torch.Tensor, stream: ctypes.c_void_p):
        """Blocks [nb, ns, 7, K] -> (the blocks in the handle's float type, their pre-folded factors or None).  float64 blocks
        for a float32 kernel object: one launch rounds them AND forms the folded factors the float32 kernels run on in
        float64, rounded once (phk_prefold; the kernels would otherwise fold the rounded rows)."""
        if x.dtype == torch.float64 and not self.double_precision and self.prefold:
            x64 = x.contiguous()
            p = torch.empty(x64.shape, dtype=torch.float32, device=self.device)
            pf = torch.empty(x64.shape[:2] + (5, self.K), dtype=torch.float32, device=self.device)
            _lib.check(_lib.load().phk_prefold(self.device.index, self.K, x64.data_ptr(), x64.shape[0] * x64.shape[1], p.data_ptr(),
                                               pf.data_ptr(), None, stream))
            return p, pf
        return x.to(self.dtype).contiguous(), None

    def _sweep_call(self, params: torch.Tensor, inds: torch.Tensor, lens: torch.Tensor | None = None) -> "_SweepCall":
        """What every sweep behind the forward pass does with ``params`` / ``inds`` / ``lens`` (as ``run`` takes them) before
        its C call: checks, padding to the compiled K, the float type of the handle."""
        assert params.is_cuda and inds.is_cuda and params.device == self.device
        assert params.ndim == 4 and params.shape[2] == 7 and params.shape[3] == self.K_user, params.shape
        B, Sp = params.shape[0], params.shape[1]
        S = inds.shape[0]
        assert inds.ndim == 1 and inds.dtype == torch.int64 and Sp in (1, S)
        params = self._pad_states(params)
        if lens is not None:
            assert lens.is_cuda and lens.device == self.device and lens.dtype == torch.int64 and lens.shape == (self.N,), "lens: int64 [N] on the device"
            lens = lens.contiguous()
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        p, pf = self._blocks(params, stream)
        inds = inds.contiguous()
        return _SweepCall(
            head=(self._h, p.data_ptr(), Sp * 7 * self.K, 7 * self.K if Sp == S else 0, pf.data_ptr() if pf is not None else None),
            grid=(inds.data_ptr(), B, S), B=B, S=S, pad_k=self.K - self.K_user, lens=lens.data_ptr() if lens is not None else None,
            stream=stream, keep=(p, pf, inds, lens),
        )

    def _nbin(self, warmup: int, bin: int) -> int:
        return (self.L - int(warmup) + int(bin) - 1) // int(bin)

    def run(self, params: torch.Tensor, inds: torch.Tensor, warmup: int = 0, grad: bool = True, dlog: bool = False):
        """params [B, S, 7, K] or [B, 1, 7, K] (one block per particle, broadcast over the chunks);
        inds int64 [S] on the device.  Returns ll [B, S] float64 and, if ``grad``, d ll/d params
        [B, S, 7, K] in the handle's float type (``dlog``: theta * d ll/d theta)."""
        assert params.is_cuda and inds.is_cuda and params.device == self.device
        assert params.ndim == 4 and params.shape[2] == 7 and params.shape[3] == self.K_user, params.shape
        params = self._pad_states(params)
        assert inds.ndim == 1 and inds.dtype == torch.int64
        B, Sp = params.shape[0], params.shape[1]
        S = inds.shape[0]
        assert Sp in (1, S)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        pf = None
        if params.dtype == torch.float64 and not self.double_precision and self.prefold:
            # float64 blocks for a float32 kernel object: one launch rounds them AND forms the folded factors the float32
            # kernels run on in float64, rounded once (phk_prefold; the kernels would otherwise fold the rounded rows)
            p64 = params.contiguous()
            p = torch.empty(p64.shape, dtype=torch.float32, device=self.device)
            pf = torch.empty((B, Sp, 5, self.K), dtype=torch.float32, device=self.device)
            # (with a gradient: also the coefficients that take the first-order effect of the rounding out of ll afterwards)
            crel = torch.empty(p64.shape, dtype=torch.float64, device=self.device) if (grad and self.first_order) else None
            _lib.check(_lib.load().phk_prefold(self.device.index, self.K, p64.data_ptr(), B * Sp, p.data_ptr(), pf.data_ptr(),
                                               crel.data_ptr() if crel is not None else None, ctypes.c_void_p(stream)))
        else:
            p = params.to(self.dtype).contiguous()
        inds = inds.contiguous()
        ll = torch.empty((B, S), dtype=torch.float64, device=self.device)
        g = torch.empty((B, S, 7, self.K), dtype=self.dtype, device=self.device) if grad else None
        stride_b = Sp * 7 * self.K
        stride_s = 7 * self.K if Sp == S else 0
        if pf is not None:
            rc = _lib.load().phk_loglik_prefolded(
                self._h, p.data_ptr(), stride_b, stride_s, pf.data_ptr(), inds.data_ptr(), B, S, int(warmup),
                ll.data_ptr(), g.data_ptr() if grad else None, int(bool(dlog)), ctypes.c_void_p(stream),
            )
        else:
            rc = _lib.load().phk_loglik(
                self._h, p.data_ptr(), stride_b, stride_s, inds.data_ptr(), B, S, int(warmup),
                ll.data_ptr(), g.data_ptr() if grad else None, int(bool(dlog)), ctypes.c_void_p(stream),
            )
        _lib.check(rc)
        if pf is not None and grad and crel is not None:
            _lib.check(_lib.load().phk_ll_first_order(self.device.index, self.K, ll.data_ptr(), g.data_ptr(), int(bool(dlog)),
                                                      p64.data_ptr(), crel.data_ptr(), stride_b, stride_s, B, S, ctypes.c_void_p(stream)))
        if grad and self.K_user != self.K:
            g = g[..., : self.K_user]
        return (ll, g) if grad else ll

    def posterior(self, params: torch.Tensor, inds: torch.Tensor, warmup: int = 0, values: torch.Tensor | None = None,
                  bin: int = 1, marginals: bool = True, mean: bool = False):
        """Posterior decoding (``phk_posterior``, the quantity of ``psmc -d``): params / inds as ``run``.  Returns
        (ll [B, S] float64, mean [B, S, nbin] or None, marginals [B, S, nbin, K] or None), the last two in the handle's float
        type, over bins of ``bin`` scored sites (nbin = ceil((L - warmup) / bin)): the bin means of gamma_t and of
        sum_k values_k gamma_t(k).  ``values`` [K] or [B, K] (float64 on the device) is required for ``mean``.  Padded
        states (K below the compiled size) get value 0 and posterior 0; they are stripped from ``marginals``."""
        assert marginals or mean, "nothing to decode: marginals and mean are both off"
        assert int(bin) >= 1 and 0 <= int(warmup) <= self.L
        c = self._sweep_call(params, inds)
        B, S = c.B, c.S
        vals, vstride = None, 0
        if mean:
            assert values is not None, "mean needs values"
            vals = torch.as_tensor(values, dtype=torch.float64, device=self.device)
            assert vals.shape[-1] == self.K_user and vals.ndim in (1, 2), vals.shape
            if vals.ndim == 2:
                assert vals.shape[0] == B
            if c.pad_k:
                vals = torch.cat([vals, vals.new_zeros(vals.shape[:-1] + (c.pad_k,))], -1)
            vals = vals.contiguous()
            vstride = self.K if vals.ndim == 2 else 0
        nbin = self._nbin(warmup, bin)
        ll = torch.empty((B, S), dtype=torch.float64, device=self.device)
        m = torch.empty((B, S, nbin), dtype=self.dtype, device=self.device) if mean else None
        g = torch.empty((B, S, nbin, self.K), dtype=self.dtype, device=self.device) if marginals else None
        rc = _lib.load().phk_posterior(
            *c.head, *c.grid, int(warmup), int(bin), vals.data_ptr() if vals is not None else None, vstride,
            ll.data_ptr(), m.data_ptr() if m is not None else None, g.data_ptr() if g is not None else None, c.stream,
        )
        _lib.check(rc)
        if g is not None and c.pad_k:
            g = g[..., : self.K_user]
        return ll, m, g

    def transitions(self, params: torch.Tensor, inds: torch.Tensor, warmup: int = 0, bin: int = 1, lens: torch.Tensor | None = None,
                    arrivals: bool = True, changes: bool = True):
        """Transition posteriors (``phk_transitions``): params / inds as ``run``.  Returns (ll [B, S] float64, changes
        [B, S, nbin, 2] or None, arrivals [B, S, nbin, 3, K] or None), the last two in the handle's float type, over bins of
        ``bin`` scored sites (nbin = ceil((L - warmup) / bin)): the bin sums of the expected moves to an older / a younger
        state and the bin means of (stay, up, down) per state.  ``lens`` (int64 [N] on the device, one own length per data
        row of the engine, ``warmup < len <= L``): sites at or past a row's own length count nothing.  Padded states (K below
        the compiled size) have no mass; they are stripped from ``arrivals``."""
        assert arrivals or changes, "nothing to compute: arrivals and changes are both off"
        assert int(bin) >= 1 and 0 <= int(warmup) <= self.L
        c = self._sweep_call(params, inds, lens)
        B, S = c.B, c.S
        nbin = self._nbin(warmup, bin)
        ll = torch.empty((B, S), dtype=torch.float64, device=self.device)
        chg = torch.empty((B, S, nbin, 2), dtype=self.dtype, device=self.device) if changes else None
        a = torch.empty((B, S, nbin, 3, self.K), dtype=self.dtype, device=self.device) if arrivals else None
        rc = _lib.load().phk_transitions(
            *c.head, *c.grid, int(warmup), int(bin), c.lens, ll.data_ptr(),
            a.data_ptr() if a is not None else None, chg.data_ptr() if chg is not None else None, c.stream,
        )
        _lib.check(rc)
        if a is not None and c.pad_k:
            a = a[..., : self.K_user]
        return ll, chg, a

    def pair_counts(self, params: torch.Tensor, inds: torch.Tensor, warmup: int = 0, lens: torch.Tensor | None = None):
        """Pair counts (``phk_pair_counts``): params / inds as ``run``.  Returns (ll [B, S] float64, counts [B, S, K, K] float64,
        origin state first): the pair posterior P(z_prev = i, z_t = j | o) summed over every row's own scored sites, the expected
        number of moves from state i to state j.  ``lens`` as ``transitions``.  Padded states (K below the compiled size) have no
        mass; they are stripped."""
        assert 0 <= int(warmup) <= self.L
        c = self._sweep_call(params, inds, lens)
        ll = torch.empty((c.B, c.S), dtype=torch.float64, device=self.device)
        counts = torch.empty((c.B, c.S, self.K, self.K), dtype=torch.float64, device=self.device)
        rc = _lib.load().phk_pair_counts(*c.head, *c.grid, int(warmup), c.lens, ll.data_ptr(), counts.data_ptr(), c.stream)
        _lib.check(rc)
        if c.pad_k:
            counts = counts[..., : self.K_user, : self.K_user]
        return ll, counts

    def predictive(self, params: torch.Tensor, inds: torch.Tensor, warmup: int = 0, bin: int = 1, lens: torch.Tensor | None = None):
        """Leave-one-out predictive decoding (``phk_predictive``): params / inds as ``run``.  Returns (ll [B, S] float64, track
        [B, S, nbin, 3] in the handle's float type) over bins of ``bin`` scored sites (nbin = ceil((L - warmup) / bin)): the
        bin sums of P(o_t = het | the row's other sites) over the observed sites, of the same over the missing sites, and of
        the log predictive of the observed sites at their own observations.  ``lens`` (int64 [N] on the device, one own length
        per data row of the engine, ``warmup < len <= L``): sites at or past a row's own length count nothing."""
        assert int(bin) >= 1 and 0 <= int(warmup) <= self.L
        c = self._sweep_call(params, inds, lens)
        nbin = self._nbin(warmup, bin)
        ll = torch.empty((c.B, c.S), dtype=torch.float64, device=self.device)
        track = torch.empty((c.B, c.S, nbin, 3), dtype=self.dtype, device=self.device)
        rc = _lib.load().phk_predictive(
            *c.head, *c.grid, int(warmup), int(bin), c.lens, ll.data_ptr(), track.data_ptr() if nbin > 0 else None, c.stream,
        )
        _lib.check(rc)
        return ll, track

    def tracts(self, params: torch.Tensor, inds: torch.Tensor, weights: torch.Tensor, warmup: int = 0, bin: int = 1,
               lens: torch.Tensor | None = None):
        """Tract posteriors (``phk_tracts``): params / inds as ``run``.  ``weights``: float64 [B, K] or [K] on the device, the
        per-state weight m in [0, 1] (an indicator of a state set for a tract probability).  Returns (ll [B, S] float64, tract
        [B, S, nbin] in the handle's float type) over bins of ``bin`` scored sites (nbin = ceil((L - warmup) / bin)): per bin
        E[prod of m(z_t) over the bin's sites | o], for an indicator the posterior probability that every site of the bin has
        its state in the set.  ``lens`` (int64 [N] on the device, one own length per data row of the engine, ``warmup < len <=
        L``): a site at or past a row's own length restricts nothing, a bin without a site of the row's own is 0."""
        assert int(bin) >= 1 and 0 <= int(warmup) <= self.L
        assert weights.is_cuda and weights.device == self.device and weights.dtype == torch.float64, "weights: float64 on the device"
        assert weights.shape in ((self.K_user,), (params.shape[0], self.K_user)), f"weights: [K] or [B, K], got {tuple(weights.shape)}"
        c = self._sweep_call(params, inds, lens)
        if c.pad_k:
            weights = torch.cat([weights, torch.zeros(weights.shape[:-1] + (c.pad_k,), dtype=weights.dtype, device=weights.device)], -1)
        weights = weights.contiguous()
        nbin = self._nbin(warmup, bin)
        ll = torch.empty((c.B, c.S), dtype=torch.float64, device=self.device)
        tract = torch.empty((c.B, c.S, nbin), dtype=self.dtype, device=self.device)
        rc = _lib.load().phk_tracts(
            *c.head, *c.grid, int(warmup), int(bin), weights.data_ptr(), self.K if weights.ndim == 2 else 0,
            c.lens, ll.data_ptr(), tract.data_ptr() if nbin > 0 else None, c.stream,
        )
        _lib.check(rc)
        return ll, tract

    def interval_tracts(self, params: torch.Tensor, inds: torch.Tensor, iv_off: torch.Tensor, iv_start: torch.Tensor,
                        iv_end: torch.Tensor, masks: torch.Tensor, warmup: int = 0, max_len: int = 1, lens: torch.Tensor | None = None):
        """Interval tracts (``phk_interval_tracts``): params / inds as ``run``.  ``iv_off`` int64 [S + 1], ``iv_start`` / ``iv_end``
        int64 [n] on the device: per chunk position the sorted, disjoint, half-open intervals ``iv_off[s] .. iv_off[s + 1] - 1`` in
        reported sites (position p is site ``warmup + p``).  ``masks``: int64 [n] or [B, n] on the device, the state set of every
        interval as a bit pattern (bit k set = state k is inside; bit 63 is the sign bit of the int64).  ``max_len``: an upper
        bound on end - start.  Returns (ll [B, S] float64, logp [B, n] float64): per interval and particle log P(every site of the
        interval has its state in the set | o).  The lists are checked on the device: one that fails raises the bad-index flag
        (``underflow_risk`` then raises) and its logp are NaN."""
        assert 0 <= int(warmup) <= self.L and int(max_len) >= 1
        c = self._sweep_call(params, inds, lens)
        n = int(iv_start.shape[0])
        for name, x, shape in (("iv_off", iv_off, (c.S + 1,)), ("iv_start", iv_start, (n,)), ("iv_end", iv_end, (n,))):
            assert x.is_cuda and x.device == self.device and x.dtype == torch.int64 and tuple(x.shape) == shape, f"{name}: int64 {shape} on the device"
        assert masks.is_cuda and masks.device == self.device and masks.dtype == torch.int64, "masks: int64 on the device"
        assert tuple(masks.shape) in ((n,), (c.B, n)), f"masks: [{n}] or [{c.B}, {n}], got {tuple(masks.shape)}"
        if c.pad_k:  # bits of the padding states (K below the compiled size) are ignored
            masks = masks & ((1 << self.K_user) - 1)
        iv_off, iv_start, iv_end, masks = iv_off.contiguous(), iv_start.contiguous(), iv_end.contiguous(), masks.contiguous()
        ll = torch.empty((c.B, c.S), dtype=torch.float64, device=self.device)
        logp = torch.empty((c.B, n), dtype=torch.float64, device=self.device)
        dummy = torch.zeros(1, dtype=torch.int64, device=self.device)  # (an empty tensor may have no address)
        rc = _lib.load().phk_interval_tracts(
            *c.head, *c.grid, int(warmup), int(max_len), c.lens, iv_off.data_ptr(), (iv_start if n else dummy).data_ptr(),
            (iv_end if n else dummy).data_ptr(), (masks if n else dummy).data_ptr(), n if masks.ndim == 2 and c.B > 1 else 0,
            ll.data_ptr(), (logp if n and c.B else dummy).data_ptr(), c.stream,
        )
        _lib.check(rc)
        return ll, logp

    def bin_moments(self, params: torch.Tensor, inds: torch.Tensor, values: torch.Tensor, warmup: int = 0, bin: int = 1,
                    lens: torch.Tensor | None = None):
        """Bin moments (``phk_bin_moments``): params / inds as ``run``.  ``values``: float64 [B, K] or [K] on the device, the
        per-state value v in [-1, 1].  Returns (ll [B, S] float64, m1 [B, S, nbin] float64, m2 [B, S, nbin] float64) over bins of
        ``bin`` scored sites (nbin = ceil((L - warmup) / bin)): per bin E[S | o] and E[S^2 | o] of S = the sum of v(z_t) over the
        bin's sites, double for either handle type.  ``lens`` (int64 [N] on the device, one own length per data row of the
        engine, ``warmup < len <= L``): a site at or past a row's own length adds nothing, a bin without a site of the row's own
        is 0.  Padded states (K below the compiled size) get value 0 and have no mass."""
        assert int(bin) >= 1 and 0 <= int(warmup) <= self.L
        assert values.is_cuda and values.device == self.device and values.dtype == torch.float64, "values: float64 on the device"
        assert values.shape in ((self.K_user,), (params.shape[0], self.K_user)), f"values: [K] or [B, K], got {tuple(values.shape)}"
        c = self._sweep_call(params, inds, lens)
        if c.pad_k:
            values = torch.cat([values, torch.zeros(values.shape[:-1] + (c.pad_k,), dtype=values.dtype, device=values.device)], -1)
        values = values.contiguous()
        nbin = self._nbin(warmup, bin)
        ll = torch.empty((c.B, c.S), dtype=torch.float64, device=self.device)
        m1 = torch.empty((c.B, c.S, nbin), dtype=torch.float64, device=self.device)
        m2 = torch.empty((c.B, c.S, nbin), dtype=torch.float64, device=self.device)
        rc = _lib.load().phk_bin_moments(
            *c.head, *c.grid, int(warmup), int(bin), values.data_ptr(), self.K if values.ndim == 2 else 0,
            c.lens, ll.data_ptr(), m1.data_ptr() if nbin > 0 else None, m2.data_ptr() if nbin > 0 else None, c.stream,
        )
        _lib.check(rc)
        return ll, m1, m2

    def local_ratio(self, params: torch.Tensor, alt: torch.Tensor, inds: torch.Tensor, warmup: int = 0, bin: int = 1,
                    lens: torch.Tensor | None = None):
        """Local likelihood-ratio scan (``phk_local_ratio``): params / inds as ``run``.  ``alt``: the alternative blocks,
        [B|1, S|1, 7, K] on the device (a leading 1 broadcasts over the particles, a second 1 over the chunks; the pi row is not
        read).  Returns (ll [B, S] float64, logratio [B, S, nbin] in the handle's float type) over bins of ``bin`` scored sites
        (nbin = ceil((L - warmup) / bin)): per bin log P(o | the bin's sites under the alternative, the rest under params) -
        log P(o | params).  ``lens`` (int64 [N] on the device, one own length per data row of the engine, ``warmup < len <=
        L``): a site at or past a row's own length is stepped with the fitted model, a bin without a site of the row's own is 0."""
        assert int(bin) >= 1 and 0 <= int(warmup) <= self.L
        c = self._sweep_call(params, inds, lens)
        B, S = c.B, c.S
        assert alt.is_cuda and alt.device == self.device
        assert alt.ndim == 4 and alt.shape[2] == 7 and alt.shape[3] == self.K_user, alt.shape
        Ba, Sa = alt.shape[0], alt.shape[1]
        assert Ba in (1, B) and Sa in (1, S), f"alt: [{B}|1, {S}|1, 7, K], got {tuple(alt.shape)}"
        a, apf = self._blocks(self._pad_states(alt), c.stream)
        nbin = self._nbin(warmup, bin)
        ll = torch.empty((B, S), dtype=torch.float64, device=self.device)
        out = torch.empty((B, S, nbin), dtype=self.dtype, device=self.device)
        rc = _lib.load().phk_local_ratio(
            *c.head, a.data_ptr(), Sa * 7 * self.K if Ba == B and B > 1 else 0, 7 * self.K if Sa == S and S > 1 else 0,
            apf.data_ptr() if apf is not None else None, *c.grid, int(warmup), int(bin),
            c.lens, ll.data_ptr(), out.data_ptr() if nbin > 0 else None, c.stream,
        )
        _lib.check(rc)
        return ll, out

    def viterbi(self, params: torch.Tensor, inds: torch.Tensor, warmup: int = 0, lens: torch.Tensor | None = None):
        """Viterbi decoding (``phk_viterbi``): params / inds as ``run``.  Returns (logp [B, S] float64, path [B, S, L - warmup]
        uint8): the log probability of the single most probable hidden path of every sequence and its states at the sites
        ``warmup .. L - 1``.  ``lens`` (int64 [N] on the device, one own length per data row of the engine, ``warmup < len <=
        L``) cuts every row at its own length: bytes of ``path`` past it are 255.  Padded states (K below the compiled size)
        are unreachable and never appear in a path."""
        assert 0 <= int(warmup) < self.L
        c = self._sweep_call(params, inds, lens)
        n_out = self.L - int(warmup)
        logp = torch.empty((c.B, c.S), dtype=torch.float64, device=self.device)
        path = torch.empty((c.B, c.S, n_out), dtype=torch.uint8, device=self.device)
        rc = _lib.load().phk_viterbi(*c.head, *c.grid, int(warmup), c.lens, logp.data_ptr(), path.data_ptr(), n_out, c.stream)
        _lib.check(rc)
        return logp, path

    def sample_paths(self, params: torch.Tensor, inds: torch.Tensor, warmup: int = 0, n_samples: int = 1, seed: int = 0):
        """Posterior path sampling (``phk_sample_paths``): params / inds as ``run``.  Returns (ll [B, S] float64, paths
        [B, S, n_samples, L - warmup] uint8): ``n_samples`` draws z ~ P(z | o) of every sequence at the sites ``warmup .. L - 1``
        (the warm-up sites condition the draws).  Draw r of sequence (b, s) of the call is a function of ``seed``, b * S + s, r
        and the site alone (a counter-based generator).  Padded states (K below the compiled size) have no mass and are never
        drawn."""
        assert 0 <= int(warmup) < self.L and 1 <= int(n_samples) <= 65535 and 0 <= int(seed) < 1 << 64
        c = self._sweep_call(params, inds)
        n_out = self.L - int(warmup)
        ll = torch.empty((c.B, c.S), dtype=torch.float64, device=self.device)
        paths = torch.empty((c.B, c.S, int(n_samples), n_out), dtype=torch.uint8, device=self.device)
        rc = _lib.load().phk_sample_paths(
            *c.head, *c.grid, int(warmup), int(n_samples), int(seed), ll.data_ptr(), paths.data_ptr(), n_out, c.stream,
        )
        _lib.check(rc)
        return ll, paths

    def sample_tracts(self, params: torch.Tensor, inds: torch.Tensor, masks: torch.Tensor, warmup: int = 0, n_samples: int = 1,
                      seed: int = 0, edges=(), lens: torch.Tensor | None = None, min_len: int = 1, bin: int | None = None):
        """Sampled tract spectra (``phk_sample_tracts``): params / inds / n_samples / seed as ``sample_paths``, whose paths this
        call draws and reduces without storing them.  ``masks``: int64 [B] or [1] on the device, the state set of every particle
        (or of all) as a bit pattern, bit k set = state k is inside (bit 63 is the sign bit of the int64).  ``edges``: up to 15
        strictly ascending tract lengths >= 1 that cut the length histogram into C = len(edges) + 1 classes (a length equal to an
        edge goes to the upper class).  ``lens`` as ``transitions``.  Returns (ll [B, S] float64, stats [B, S, n_samples, 4 + C]
        int32, cover [B, S, nbin] int32 or None): per sample the own reported sites inside the set, the number of tracts, the
        longest tract, the changes of state and the histogram; with ``bin`` given, per bin of ``bin`` reported sites the number
        of own sites, summed over the samples, that lie in a tract of at least ``min_len`` sites."""
        assert 0 <= int(warmup) < self.L and 1 <= int(n_samples) <= 65535 and 0 <= int(seed) < 1 << 64
        edges = [int(e) for e in edges]
        assert len(edges) <= 15 and all(e >= 1 for e in edges) and all(a < b for a, b in zip(edges, edges[1:])), \
            f"edges: at most 15 strictly ascending lengths >= 1, got {edges}"
        assert masks.is_cuda and masks.device == self.device and masks.dtype == torch.int64, "masks: int64 on the device"
        assert masks.shape in ((1,), (params.shape[0],)), f"masks: [1] or [B], got {tuple(masks.shape)}"
        c = self._sweep_call(params, inds, lens)
        masks = masks.contiguous()
        C = len(edges) + 1
        ll = torch.empty((c.B, c.S), dtype=torch.float64, device=self.device)
        stats = torch.empty((c.B, c.S, int(n_samples), 4 + C), dtype=torch.int32, device=self.device)
        cover = None
        if bin is not None:
            assert int(bin) >= 1 and int(min_len) >= 1
            assert int(n_samples) * min(int(bin), self.L - int(warmup)) < 1 << 31, "n_samples x bin does not fit the int32 cover"
            cover = torch.empty((c.B, c.S, self._nbin(warmup, bin)), dtype=torch.int32, device=self.device)
        earr = (ctypes.c_int64 * max(len(edges), 1))(*edges)
        rc = _lib.load().phk_sample_tracts(
            *c.head, *c.grid, int(warmup), int(n_samples), int(seed), masks.data_ptr(), 1 if masks.shape[0] == c.B and c.B > 1 else 0,
            c.lens, earr, len(edges), int(bin) if bin is not None else 1, int(min_len), ll.data_ptr(), stats.data_ptr(),
            cover.data_ptr() if cover is not None else None, c.stream,
        )
        _lib.check(rc)
        return ll, stats, cover
