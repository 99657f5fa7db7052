"""Decoding of whole contigs: the posterior mean TMRCA along the genome (what ``psmc -d`` reports), under one fitted model
or averaged over the posterior sample ``fit`` returns, the most probable TMRCA path (Viterbi) with its segments, and TMRCA
paths drawn from the posterior.

The HMM posteriors come from the decode sweep of the HIP engine (``PSMCKernel.posterior`` -> ``phk_posterior``), the paths
from its Viterbi kernels (``PSMCKernel.viterbi`` -> ``phk_viterbi``) and its sampling traceback (``PSMCKernel.sample_paths`` ->
``phk_sample_paths``), the breakpoint track from its transition sweep (``PSMCKernel.transitions`` -> ``phk_transitions``) and
the leave-one-out check of the observations from its predictive sweep (``PSMCKernel.predictive`` -> ``phk_predictive``) and the
tract probabilities from its tract sweep (``PSMCKernel.tracts`` -> ``phk_tracts``) and the local likelihood-ratio scans from its
local-ratio sweep (``PSMCKernel.local_ratio`` -> ``phk_local_ratio``) and the expected transition matrix from its pair-count sweep
(``PSMCKernel.pair_counts`` -> ``phk_pair_counts``) and the error band of the TMRCA track from its bin-moment sweep
(``PSMCKernel.bin_moments`` -> ``phk_bin_moments``) and the tract-length spectra from its reducing sampling traceback
(``PSMCKernel.sample_tracts`` -> ``phk_sample_tracts``); this module only builds the models, pads ragged inputs,
averages, counts and run-length encodes.  There is no CPU path to the kernels' results; ``path_tracts`` is plain torch on paths
a caller already holds.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from .data import RawContig
from .kernel import PSMCKernel
from .params import PSMCParams
from .size_history import DemographicModel, SizeHistory


def _rows(data):
    """-> (int8 [N, Lmax] padded with -1, list of (first row, rows, length) per contig, or None for a plain matrix)"""
    if isinstance(data, (list, tuple)):
        mats = []
        for c in data:
            m = c.het_matrix if isinstance(c, RawContig) else c
            m = np.asarray(m)
            mats.append(m[None] if m.ndim == 1 else m)
        Lmax = max(m.shape[1] for m in mats)
        out = np.full((sum(m.shape[0] for m in mats), Lmax), -1, dtype=np.int8)
        spans, r = [], 0
        for m in mats:
            out[r : r + m.shape[0], : m.shape[1]] = m
            spans.append((r, m.shape[0], m.shape[1]))
            r += m.shape[0]
        return out, spans
    if isinstance(data, torch.Tensor):
        data = data.cpu().numpy()
    d = np.asarray(data)
    assert d.ndim == 2 and d.dtype == np.int8, "data: int8 [N, L] het matrix (or a list of RawContig)"
    return d, None


def posterior_tmrca(dms, data, window_size: int = 100, bin: int = 1, device=None, double_precision: bool = False):
    """Posterior mean TMRCA per bin of ``bin`` windows, for every row of ``data``.

    dms: one ``DemographicModel`` or the list ``fit()`` returns, with theta and rho per base pair; every model is evaluated
        with theta and rho times ``window_size`` (per window) and the states' expected coalescence times ``dm.eta.ect()``,
        in the model's own time unit (generations when ``fit`` was given ``mutation_rate``), and the tracks are averaged
        with equal weight.
    data: int8 [N, L] het matrix of whole-contig rows (-1 missing, 0 hom, 1 het), or a list of ``RawContig`` (or of
        int8 matrices) of different lengths: they are padded with missing windows and the padding is stripped again.
    Returns float64 [N, ceil(L / bin)] on the device for a matrix, a list of such tensors (one per contig) for a list.
    """
    if isinstance(dms, DemographicModel):
        dms = [dms]
    dms = list(dms)
    assert len(dms) > 0, "no model to decode under"
    M = dms[0].M
    assert all(dm.M == M for dm in dms), "all models must have the same number of states"
    if isinstance(data, (list, tuple)):
        for c in data:
            if isinstance(c, RawContig):
                c.get_data(window_size)  # (raises if the contig was built with another window size)
    rows, spans = _rows(data)
    kern = PSMCKernel(M, rows, double_precision=double_precision, device=device)
    dev = kern.device
    per = [DemographicModel(eta=dm.eta, theta=float(dm.theta) * window_size, rho=float(dm.rho) * window_size) for dm in dms]
    pps = [PSMCParams.from_dm(dm) for dm in per]
    pp = PSMCParams(*(torch.stack([torch.as_tensor(getattr(p, f), dtype=torch.float64) for p in pps])[:, None]
                      for f in PSMCParams._fields))  # [B, 1, M]: one block per model, broadcast over the rows
    values = torch.stack([torch.as_tensor(dm.eta.ect(), dtype=torch.float64) for dm in dms]).to(dev)  # [B, M]
    inds = torch.arange(rows.shape[0], device=dev)
    out = kern.posterior(pp, inds, values=values, bin=bin, marginals=False)
    track = out.mean.to(torch.float64).mean(0)  # [N, nbin]: equal weight per model
    if spans is None:
        return track
    return [track[r : r + n, : (length + bin - 1) // bin] for r, n, length in spans]


def posterior_changes(dms, data, window_size: int = 100, bin: int = 1, device=None, double_precision: bool = False):
    """Expected number of TMRCA changes per bin of ``bin`` windows, for every row of ``data``: the breakpoint track.

    For each bin, (moves to an older state, moves to a younger state): the sums over the bin's windows of
    P(z_prev < z_t | o) and P(z_prev > z_t | o), exact (``PSMCKernel.transitions``), not estimated from sampled paths.  A
    change is a change of the TMRCA state; a recombination that coalesces again in the same interval is not one.

    dms: one ``DemographicModel`` or the list ``fit()`` returns, evaluated per window as in ``posterior_tmrca``; the tracks
        are averaged with equal weight.
    data: int8 [N, L] het matrix of whole-contig rows (-1 missing, 0 hom, 1 het), or a list of ``RawContig`` (or of int8
        matrices) of different lengths: they are padded with missing windows, and the padded windows count nothing (each
        row's own length goes to the kernel, which masks them: a padded window would otherwise add the prior's change rate).
    Returns float64 [N, ceil(L / bin), 2] on the device for a matrix, a list of such tensors (one per contig) for a list.
    """
    if isinstance(dms, DemographicModel):
        dms = [dms]
    dms = list(dms)
    assert len(dms) > 0, "no model to decode under"
    M = dms[0].M
    assert all(dm.M == M for dm in dms), "all models must have the same number of states"
    if isinstance(data, (list, tuple)):
        for c in data:
            if isinstance(c, RawContig):
                c.get_data(window_size)  # (raises if the contig was built with another window size)
    rows, spans = _rows(data)
    lens = None
    if spans is not None:
        lens = np.concatenate([np.full(n, length, dtype=np.int64) for _, n, length in spans])
    kern = PSMCKernel(M, rows, double_precision=double_precision, device=device)
    dev = kern.device
    per = [DemographicModel(eta=dm.eta, theta=float(dm.theta) * window_size, rho=float(dm.rho) * window_size) for dm in dms]
    pps = [PSMCParams.from_dm(dm) for dm in per]
    pp = PSMCParams(*(torch.stack([torch.as_tensor(getattr(p, f), dtype=torch.float64) for p in pps])[:, None]
                      for f in PSMCParams._fields))  # [B, 1, M]: one block per model, broadcast over the rows
    out = kern.transitions(pp, torch.arange(rows.shape[0], device=dev), bin=bin, lens=lens, arrivals=False)
    track = out.changes.to(torch.float64).mean(0)  # [N, nbin, 2]: equal weight per model
    if spans is None:
        return track
    return [track[r : r + n, : (length + bin - 1) // bin] for r, n, length in spans]


def predictive_check(dms, data, window_size: int = 100, bin: int = 1, device=None, double_precision: bool = False):
    """Leave-one-out check of a size history along the genome, per bin of ``bin`` windows, for every row of ``data``: what the
    model expects of each window given all the others, beside what the data has.

    For each bin five numbers: (expected het windows among the observed ones, imputed het windows among the missing ones, the
    leave-one-out log score, observed het windows, observed windows).  The first three are bin sums of phet_t = P(window t is
    het | every other window of the row) over the observed windows, of the same over the missing windows, and of
    log P(o_t | o_{-t}) over the observed windows, exact (``PSMCKernel.predictive``); the last two are counted from ``data``
    on the host.  Where the first runs far from the fourth the model predicts the data badly; the second is the imputation
    under an accessibility mask.

    dms: one ``DemographicModel`` or the list ``fit()`` returns, evaluated per window as in ``posterior_tmrca``.  The first
        three numbers are averaged over the models with equal weight.  The mean over models of per-model leave-one-out terms
        is NOT the leave-one-out predictive of the mixture of the models: that one averages phet_t per site before the log is
        taken, which this function does not do.
    data: int8 [N, L] het matrix of whole-contig rows (-1 missing, 0 hom, 1 het), or a list of ``RawContig`` (or of int8
        matrices) of different lengths: they are padded with missing windows, and the padded windows count nothing (each
        row's own length goes to the kernel, which masks them: a padded window would otherwise be imputed).
    Returns float64 [N, ceil(L / bin), 5] on the device for a matrix, a list of such tensors (one per contig) for a list.
    """
    if isinstance(dms, DemographicModel):
        dms = [dms]
    dms = list(dms)
    assert len(dms) > 0, "no model to decode under"
    M = dms[0].M
    assert all(dm.M == M for dm in dms), "all models must have the same number of states"
    if isinstance(data, (list, tuple)):
        for c in data:
            if isinstance(c, RawContig):
                c.get_data(window_size)  # (raises if the contig was built with another window size)
    rows, spans = _rows(data)
    lens = None
    if spans is not None:
        lens = np.concatenate([np.full(n, length, dtype=np.int64) for _, n, length in spans])
    kern = PSMCKernel(M, rows, double_precision=double_precision, device=device)
    dev = kern.device
    per = [DemographicModel(eta=dm.eta, theta=float(dm.theta) * window_size, rho=float(dm.rho) * window_size) for dm in dms]
    pps = [PSMCParams.from_dm(dm) for dm in per]
    pp = PSMCParams(*(torch.stack([torch.as_tensor(getattr(p, f), dtype=torch.float64) for p in pps])[:, None]
                      for f in PSMCParams._fields))  # [B, 1, M]: one block per model, broadcast over the rows
    out = kern.predictive(pp, torch.arange(rows.shape[0], device=dev), bin=bin, lens=lens)
    model = torch.stack([out.het_observed, out.het_missing, out.score], -1).to(torch.float64).mean(0)  # [N, nbin, 3]
    # the data's own counts per bin (padding is missing: it counts nothing)
    N, L = rows.shape
    nbin = (L + bin - 1) // bin
    padded = np.full((N, nbin * bin), -1, dtype=np.int8)
    padded[:, :L] = rows
    padded = padded.reshape(N, nbin, bin)
    own = np.stack([(padded >= 1).sum(-1), (padded >= 0).sum(-1)], -1).astype(np.float64)
    track = torch.cat([model, torch.as_tensor(own, device=dev)], -1)  # [N, nbin, 5]
    if spans is None:
        return track
    return [track[r : r + n, : (length + bin - 1) // bin] for r, n, length in spans]


def _range_sets(dms, t_min, t_max) -> np.ndarray:
    """bool [len(dms), M]: per model the states whose whole interval [eta.t[k], eta.t[k + 1]) (the last one open) lies inside
    [t_min, t_max)"""
    assert float(t_min) < float(t_max), "the TMRCA range [t_min, t_max) is empty"
    M = dms[0].M
    w = np.empty((len(dms), M), dtype=bool)
    for i, dm in enumerate(dms):
        t = np.asarray(torch.as_tensor(dm.eta.t, dtype=torch.float64).cpu().numpy(), dtype=np.float64).reshape(M)
        lo, hi = t, np.append(t[1:], np.inf)
        w[i] = (lo >= float(t_min)) & (hi <= float(t_max))
    return w


def tract_posterior(dms, data, t_max, t_min: float = 0.0, window_size: int = 100, bin: int = 1, weights=None, device=None,
                    double_precision: bool = False):
    """Posterior probability that the TMRCA of EVERY window of a bin of ``bin`` windows lies in [t_min, t_max), for every row of
    ``data``: where the tracts are (``t_max`` small: runs of homozygosity and IBD segments; ``t_min`` large: deep-coalescence
    deserts).  The event is joint over the bin's windows and the probability is exact (``PSMCKernel.tracts``): the bin mean of the
    per-window marginals is only an upper bound of it, and sampled paths only estimate it.

    dms: one ``DemographicModel`` or the list ``fit()`` returns, evaluated per window as in ``posterior_tmrca``.  For each model,
        state k covers [eta.t[k], eta.t[k + 1]), the last one open, in the model's own time unit (that of ``eta.ect()``:
        generations when ``fit`` was given ``mutation_rate``); the state counts as inside when its whole interval lies inside
        [t_min, t_max).  The probabilities are averaged over the models with equal weight, and this mean IS the posterior
        probability of the event under the equal-weight mixture of the models: a probability given the data is linear in the
        mixture's components (unlike the leave-one-out terms of ``predictive_check``).
    data: int8 [N, L] het matrix of whole-contig rows (-1 missing, 0 hom, 1 het), or a list of ``RawContig`` (or of int8
        matrices) of different lengths: they are padded with missing windows, and the padded windows restrict nothing (each
        row's own length goes to the kernel, which masks them).
    weights: [M] or [len(dms), M] in [0, 1], overriding the time range: the result is then E[prod of weights(z_t) over the
        bin's windows | data].
    Returns float64 [N, ceil(L / bin)] on the device for a matrix, a list of such tensors (one per contig) for a list.
    """
    if isinstance(dms, DemographicModel):
        dms = [dms]
    dms = list(dms)
    assert len(dms) > 0, "no model to decode under"
    M = dms[0].M
    assert all(dm.M == M for dm in dms), "all models must have the same number of states"
    if weights is None:
        w = _range_sets(dms, t_min, t_max).astype(np.float64)
    else:
        w = np.asarray(weights.cpu() if isinstance(weights, torch.Tensor) else weights, dtype=np.float64)
        assert w.shape in ((M,), (len(dms), M)), f"weights: [{M}] or [{len(dms)}, {M}]"
    if isinstance(data, (list, tuple)):
        for c in data:
            if isinstance(c, RawContig):
                c.get_data(window_size)  # (raises if the contig was built with another window size)
    rows, spans = _rows(data)
    lens = None
    if spans is not None:
        lens = np.concatenate([np.full(n, length, dtype=np.int64) for _, n, length in spans])
    kern = PSMCKernel(M, rows, double_precision=double_precision, device=device)
    dev = kern.device
    per = [DemographicModel(eta=dm.eta, theta=float(dm.theta) * window_size, rho=float(dm.rho) * window_size) for dm in dms]
    pps = [PSMCParams.from_dm(dm) for dm in per]
    pp = PSMCParams(*(torch.stack([torch.as_tensor(getattr(p, f), dtype=torch.float64) for p in pps])[:, None]
                      for f in PSMCParams._fields))  # [B, 1, M]: one block per model, broadcast over the rows
    out = kern.tracts(pp, torch.arange(rows.shape[0], device=dev), weights=w, bin=bin, lens=lens)
    track = out.prob.to(torch.float64).mean(0)  # [N, nbin]: equal weight per model
    if spans is None:
        return track
    return [track[r : r + n, : (length + bin - 1) // bin] for r, n, length in spans]


class TmrcaBand(NamedTuple):
    """What ``tmrca_band`` returns: float64 tensors on the device for a matrix, lists with one tensor per contig for a list."""

    mean: torch.Tensor  # [N, nbin]: the posterior mean of the bin-mean value, averaged over the models
    sd: torch.Tensor  # [N, nbin]: its posterior standard deviation under the equal-weight mixture of the models
    sd_within: torch.Tensor  # [N, nbin]: the part of sd from the unknown path (root of the mean of the per-model variances)
    sd_between: torch.Tensor  # [N, nbin]: the part of sd from the unknown size history (sd of the per-model means)


def tmrca_band(dms, data, window_size: int = 100, bin: int = 100, values=None, device=None, double_precision: bool = False):
    """The track of ``posterior_tmrca`` with its error bar: per bin of ``bin`` windows, for every row of ``data``, the posterior
    mean and standard deviation of the bin-MEAN value S / n, S = the sum over the bin's n windows of ``values``(z_t).  The
    variance is exact (``PSMCKernel.bin_moments``) and holds the covariances between a bin's windows, which dominate it:
    neighbouring windows share their TMRCA, so the per-window marginals would give far too narrow a band.

    dms: one ``DemographicModel`` or the list ``fit()`` returns, evaluated per window as in ``posterior_tmrca``.  Raw moments
        are linear in a mixture, so under the equal-weight mixture of the models the variance splits by the law of total
        variance: ``sd_within``^2 = the mean of the per-model variances (the path is unknown), ``sd_between``^2 = the variance of
        the per-model means (the size history is unknown), ``sd``^2 = their sum; ``mean`` = the mean of the per-model means.  All
        four are formed from per-model means and variances in float64; no two large squares are subtracted.
    data: int8 [N, L] het matrix of whole-contig rows (-1 missing, 0 hom, 1 het), or a list of ``RawContig`` (or of int8
        matrices) of different lengths: they are padded with missing windows, and the padded windows add nothing (each row's own
        length goes to the kernel, which masks them; a partial last bin is averaged over its own windows).
    values: None for each model's ``eta.ect()`` (the TMRCA, in the model's own time unit), or [M] or [len(dms), M]: a value per
        state, e.g. the indicator of a TMRCA range for the share of a bin's windows inside it.
    Returns ``TmrcaBand(mean, sd, sd_within, sd_between)``: float64 [N, ceil(L / bin)] on the device for a matrix, lists of such
    tensors (one per contig) for a list.
    """
    if isinstance(dms, DemographicModel):
        dms = [dms]
    dms = list(dms)
    assert len(dms) > 0, "no model to decode under"
    M = dms[0].M
    assert all(dm.M == M for dm in dms), "all models must have the same number of states"
    if values is None:
        v = np.stack([np.asarray(torch.as_tensor(dm.eta.ect(), dtype=torch.float64).cpu().numpy(), dtype=np.float64).reshape(M) for dm in dms])
    else:
        v = np.asarray(values.cpu() if isinstance(values, torch.Tensor) else values, dtype=np.float64)
        assert v.shape in ((M,), (len(dms), M)), f"values: [{M}] or [{len(dms)}, {M}]"
    if isinstance(data, (list, tuple)):
        for c in data:
            if isinstance(c, RawContig):
                c.get_data(window_size)  # (raises if the contig was built with another window size)
    rows, spans = _rows(data)
    N, L = rows.shape
    lens = np.full(N, L, dtype=np.int64)
    if spans is not None:
        lens = np.concatenate([np.full(n, length, dtype=np.int64) for _, n, length in spans])
    kern = PSMCKernel(M, rows, double_precision=double_precision, device=device)
    dev = kern.device
    per = [DemographicModel(eta=dm.eta, theta=float(dm.theta) * window_size, rho=float(dm.rho) * window_size) for dm in dms]
    pps = [PSMCParams.from_dm(dm) for dm in per]
    pp = PSMCParams(*(torch.stack([torch.as_tensor(getattr(p, f), dtype=torch.float64) for p in pps])[:, None]
                      for f in PSMCParams._fields))  # [B, 1, M]: one block per model, broadcast over the rows
    out = kern.bin_moments(pp, torch.arange(N, device=dev), values=v, bin=bin, lens=lens if spans is not None else None)
    # the bin's own windows (at least 1 in every bin that is returned)
    nbin = (L + bin - 1) // bin
    n = np.clip(lens[:, None] - np.arange(nbin)[None, :] * bin, 1, bin).astype(np.float64)
    n = torch.as_tensor(n, device=dev)
    mu = out.mean / n  # [B, N, nbin]: per model
    var = out.var / (n * n)
    mean = mu.mean(0)
    within = var.mean(0)
    between = ((mu - mean) ** 2).mean(0)
    tracks = (mean, torch.sqrt(within + between), torch.sqrt(within), torch.sqrt(between))
    if spans is None:
        return TmrcaBand(*tracks)
    return TmrcaBand(*([t[r : r + k, : (length + bin - 1) // bin] for r, k, length in spans] for t in tracks))


class LocalScan(NamedTuple):
    """What ``local_scan`` returns: tensors on the device for a matrix, lists with one tensor per contig for a list."""

    log_ratio: torch.Tensor  # float64 [N, nbin, J]: per row, bin and scale, the mean over the models of the per-model log ratios
    composite: torch.Tensor  # float64 [nbin, J]: the sum of log_ratio over the rows (of the contig)
    scales: tuple  # the J scales, ascending, 1.0 among them
    best: torch.Tensor  # float64 [nbin]: the scale with the largest composite


def local_scan(dms, data, what: str = "theta", scales=(0.25, 0.5, 2.0, 4.0), window_size: int = 100, bin: int = 100, device=None,
               double_precision: bool = False):
    """Where along the genome the fitted model is wrong, and in which direction: a per-bin profile likelihood over a scale of the
    mutation rate, the recombination rate or the population size.  For every bin of ``bin`` windows and every scale s,
    log P(data | the bin's windows generated by the model with ``what`` times s, the rest of the row by the model itself) -
    log P(data | the model), exact (``PSMCKernel.local_ratio``, one sweep per scale): a window of doubled mutation rate, a
    recombination cold spot, a region of reduced local Ne (background selection, a sweep).

    dms: one ``DemographicModel`` or the list ``fit()`` returns, evaluated per window as in ``posterior_tmrca``.  The log ratios
        are averaged over the models with equal weight: that mean is the posterior expectation of the log likelihood ratio over
        the ``fit()`` sample, NOT the log ratio of the mixture of the models (which would average the likelihoods before the log
        is taken).
    data: int8 [N, L] het matrix of whole-contig rows (-1 missing, 0 hom, 1 het), or a list of ``RawContig`` (or of int8
        matrices) of different lengths: they are padded with missing windows, the padded windows belong to no alternative (each
        row's own length goes to the kernel, which masks them) and are cut away again.
    what: ``"theta"`` (the alternative has theta times s), ``"rho"`` (rho times s) or ``"ne"`` (``eta.c / s`` on the same time
        grid: the population size times s).
    scales: the scales to try; 1 is always part of the result, as the column of exact zeros, and costs no sweep.
    Returns ``LocalScan(log_ratio, composite, scales, best)``: ``log_ratio`` float64 [N, nbin, J] with nbin = ceil(L / bin) and J
    the number of scales (``scales``, ascending); ``composite`` [nbin, J], its sum over the rows: the scan of a cohort of pairs
    treated as a composite likelihood, and the quantity to look at -- a single row's scan is confounded by the local TMRCA (a
    deep local genealogy looks like a raised mutation rate), which differs from pair to pair while a property of the region does
    not; ``best`` [nbin], the scale with the largest composite.  For a list of contigs the three are lists with one tensor per
    contig (rows, bins and composite of that contig alone).
    """
    assert what in ("theta", "rho", "ne"), 'what: "theta", "rho" or "ne"'
    if isinstance(dms, DemographicModel):
        dms = [dms]
    dms = list(dms)
    assert len(dms) > 0, "no model to decode under"
    M = dms[0].M
    assert all(dm.M == M for dm in dms), "all models must have the same number of states"
    sc = sorted({float(s) for s in scales} | {1.0})
    assert all(np.isfinite(s) and s > 0 for s in sc), "scales must be positive and finite"
    if isinstance(data, (list, tuple)):
        for c in data:
            if isinstance(c, RawContig):
                c.get_data(window_size)  # (raises if the contig was built with another window size)
    rows, spans = _rows(data)
    lens = None
    if spans is not None:
        lens = np.concatenate([np.full(n, length, dtype=np.int64) for _, n, length in spans])
    kern = PSMCKernel(M, rows, double_precision=double_precision, device=device)
    dev = kern.device

    def blocks(models):  # [B, 1, M] fields: one block per model, broadcast over the rows
        pps = [PSMCParams.from_dm(dm) for dm in models]
        return PSMCParams(*(torch.stack([torch.as_tensor(getattr(p, f), dtype=torch.float64) for p in pps])[:, None]
                            for f in PSMCParams._fields))

    def scaled(dm, s):
        theta, rho, eta = float(dm.theta) * window_size, float(dm.rho) * window_size, dm.eta
        if what == "theta":
            theta *= s
        elif what == "rho":
            rho *= s
        else:
            eta = SizeHistory(t=eta.t, c=torch.as_tensor(eta.c, dtype=torch.float64) / s)
        return DemographicModel(eta=eta, theta=theta, rho=rho)

    pp = blocks([scaled(dm, 1.0) for dm in dms])
    inds = torch.arange(rows.shape[0], device=dev)
    N, nbin = rows.shape[0], (rows.shape[1] + bin - 1) // bin
    lr = torch.zeros((N, nbin, len(sc)), dtype=torch.float64, device=dev)
    for j, s in enumerate(sc):
        if s == 1.0:
            continue  # (the alternative is the model itself: exactly 0)
        out = kern.local_ratio(pp, blocks([scaled(dm, s) for dm in dms]), inds, bin=bin, lens=lens)
        lr[:, :, j] = out.log_ratio.to(torch.float64).mean(0)  # equal weight per model
    sct = torch.tensor(sc, dtype=torch.float64, device=dev)
    if spans is None:
        comp = lr.sum(0)
        return LocalScan(lr, comp, tuple(sc), sct[comp.argmax(-1)])
    lrs = [lr[r : r + n, : (length + bin - 1) // bin] for r, n, length in spans]
    comps = [x.sum(0) for x in lrs]
    return LocalScan(lrs, comps, tuple(sc), [sct[c.argmax(-1)] for c in comps])


class TransitionCounts(NamedTuple):
    """What ``transition_counts`` returns: float64 tensors on the device, origin state first."""

    counts: torch.Tensor  # [M, M]: the mean over the models of per_model
    expected: torch.Tensor  # [M, M]: the mean over the models of (row sums of per_model) * the model's own transition matrix
    per_model: torch.Tensor  # [n_models, M, M]: expected moves from state i to state j, summed over every row of every contig


def _dense_transition(pp: PSMCParams) -> torch.Tensor:
    """[..., M, M] transition matrix of SMC' from its structured factors: b_j below the diagonal, d_j on it, u_i v_j above"""
    b, d, u, v = (torch.as_tensor(getattr(pp, f), dtype=torch.float64) for f in ("b", "d", "u", "v"))
    below = torch.tril(b[..., None, :].expand(b.shape + b.shape[-1:]), -1)
    return below + torch.diag_embed(d) + torch.triu(u[..., :, None] * v[..., None, :], 1)


def transition_counts(dms, data, window_size: int = 100, device=None, double_precision: bool = False) -> TransitionCounts:
    """The expected M x M matrix of TMRCA-state transitions over all of ``data``, beside what the model's own transition kernel
    would give: a calibration of the SMC' transition structure that does not depend on the emission check of
    ``predictive_check``.

    ``per_model[m, i, j]`` is the sum over every window of every row of P(z_prev = i, z_t = j | data) under model m, exact
    (``PSMCKernel.pair_counts``): the expected number of moves from state i to state j, and the Baum-Welch transition statistic.
    ``counts`` is its mean over the models.  ``expected`` is the mean over the models of rowsum_i(per_model) * A_model[i, j]:
    what the model's transition matrix makes of the same posterior occupancy of the origin states.  ``counts / expected`` far
    from 1 in row i says the data moves away from state i differently than the model does.  Both matrices sum to the number
    of windows in ``data``.  The diagonal counts windows whose state stays: a recombination that coalesces again in the same
    interval is not a move.

    dms: one ``DemographicModel`` or the list ``fit()`` returns, evaluated per window as in ``posterior_tmrca``.
    data: int8 [N, L] het matrix of whole-contig rows (-1 missing, 0 hom, 1 het), or a list of ``RawContig`` (or of int8
        matrices) of different lengths: they are padded with missing windows, and the padded windows count nothing (each row's
        own length goes to the kernel, which masks them).
    Returns ``TransitionCounts(counts, expected, per_model)``, float64 on the device.
    """
    if isinstance(dms, DemographicModel):
        dms = [dms]
    dms = list(dms)
    assert len(dms) > 0, "no model to decode under"
    M = dms[0].M
    assert all(dm.M == M for dm in dms), "all models must have the same number of states"
    if isinstance(data, (list, tuple)):
        for c in data:
            if isinstance(c, RawContig):
                c.get_data(window_size)  # (raises if the contig was built with another window size)
    rows, spans = _rows(data)
    lens = None
    if spans is not None:
        lens = np.concatenate([np.full(n, length, dtype=np.int64) for _, n, length in spans])
    kern = PSMCKernel(M, rows, double_precision=double_precision, device=device)
    dev = kern.device
    per = [DemographicModel(eta=dm.eta, theta=float(dm.theta) * window_size, rho=float(dm.rho) * window_size) for dm in dms]
    pps = [PSMCParams.from_dm(dm) for dm in per]
    pp = PSMCParams(*(torch.stack([torch.as_tensor(getattr(p, f), dtype=torch.float64) for p in pps])[:, None]
                      for f in PSMCParams._fields))  # [B, 1, M]: one block per model, broadcast over the rows
    out = kern.pair_counts(pp, torch.arange(rows.shape[0], device=dev), lens=lens)
    per_model = out.counts.to(torch.float64).sum(1)  # [B, M, M]: every row of every contig
    A = _dense_transition(PSMCParams(*(f[:, 0] for f in pp))).to(per_model.device)  # [B, M, M]
    expected = (per_model.sum(-1, keepdim=True) * A).mean(0)
    return TransitionCounts(per_model.mean(0), expected, per_model)


def viterbi_tmrca(dm, data, window_size: int = 100, device=None, double_precision: bool = False):
    """The most probable hidden path (Viterbi) of every row of ``data`` and its TMRCA track.

    dm: one ``DemographicModel`` or a list of them (one path per model: most probable paths are not averaged), with theta
        and rho per base pair, evaluated per window as in ``posterior_tmrca``.
    data: int8 [N, L] het matrix of whole-contig rows, or a list of ``RawContig`` (or of int8 matrices) of different
        lengths.  Ragged rows are decoded at their own lengths (a missing tail would bend the end of the path), not padded.
    Returns ``(path, tmrca)``: the states (uint8) and ``dm.eta.ect()[path]`` (float64, the model's own time unit), on the
    device.  For a matrix: [N, L] ([B, N, L] for a list of B models); for a list of contigs: a list with one such tensor
    per contig, cut to the contig's length.
    """
    single = isinstance(dm, DemographicModel)
    dms = [dm] if single else list(dm)
    assert len(dms) > 0, "no model to decode under"
    M = dms[0].M
    assert all(m.M == M for m in dms), "all models must have the same number of states"
    if isinstance(data, (list, tuple)):
        for c in data:
            if isinstance(c, RawContig):
                c.get_data(window_size)  # (raises if the contig was built with another window size)
    rows, spans = _rows(data)
    lens = None
    if spans is not None:
        lens = np.concatenate([np.full(n, length, dtype=np.int64) for _, n, length in spans])
    kern = PSMCKernel(M, rows, double_precision=double_precision, device=device)
    dev = kern.device
    per = [DemographicModel(eta=m.eta, theta=float(m.theta) * window_size, rho=float(m.rho) * window_size) for m in dms]
    pps = [PSMCParams.from_dm(m) for m in per]
    pp = PSMCParams(*(torch.stack([torch.as_tensor(getattr(p, f), dtype=torch.float64) for p in pps])[:, None]
                      for f in PSMCParams._fields))  # [B, 1, M]: one block per model, broadcast over the rows
    values = torch.stack([torch.as_tensor(m.eta.ect(), dtype=torch.float64) for m in dms]).to(dev)  # [B, M]
    out = kern.viterbi(pp, torch.arange(rows.shape[0], device=dev), lens=lens)
    path = out.path  # [B, N, L]
    idx = path.long().clamp_(max=M - 1)  # (255 past a row's own length: cut away below)
    track = torch.gather(values[:, None, :].expand(-1, path.shape[1], -1), 2, idx)
    if single:
        path, track = path[0], track[0]
    if spans is None:
        return path, track
    return ([path[..., r : r + n, :length] for r, n, length in spans], [track[..., r : r + n, :length] for r, n, length in spans])


def sample_tmrca(dms, data, n_samples: int = 1, seed: int = 0, window_size: int = 100, device=None, double_precision: bool = False):
    """Hidden paths drawn from the posterior, z ~ P(z | o), of every row of ``data``, and their TMRCA tracks.

    dms: one ``DemographicModel`` or a list of B of them (e.g. what ``fit()`` returns: ``n_samples`` paths per model are then
        draws from the joint posterior over size history and path), with theta and rho per base pair, evaluated per window as
        in ``posterior_tmrca``.
    data: int8 [N, L] het matrix of whole-contig rows, or a list of ``RawContig`` (or of int8 matrices) of different
        lengths: they are padded with missing windows and the padding is cut away again (unlike a most probable path, a
        draw over the padded row has exactly the right distribution on the row's own sites).
    Returns ``(paths, tmrca)``: the states (uint8) and ``dm.eta.ect()[paths]`` (float64, the model's own time unit), on the
    device.  For a matrix: [N, n_samples, L] ([B, N, n_samples, L] for a list of B models); for a list of contigs: a list with
    one such tensor per contig, cut to the contig's length.  The same ``seed`` gives the same paths.
    """
    single = isinstance(dms, DemographicModel)
    dms = [dms] if single else list(dms)
    assert len(dms) > 0, "no model to sample under"
    M = dms[0].M
    assert all(m.M == M for m in dms), "all models must have the same number of states"
    if isinstance(data, (list, tuple)):
        for c in data:
            if isinstance(c, RawContig):
                c.get_data(window_size)  # (raises if the contig was built with another window size)
    rows, spans = _rows(data)
    kern = PSMCKernel(M, rows, double_precision=double_precision, device=device)
    dev = kern.device
    per = [DemographicModel(eta=m.eta, theta=float(m.theta) * window_size, rho=float(m.rho) * window_size) for m in dms]
    pps = [PSMCParams.from_dm(m) for m in per]
    pp = PSMCParams(*(torch.stack([torch.as_tensor(getattr(p, f), dtype=torch.float64) for p in pps])[:, None]
                      for f in PSMCParams._fields))  # [B, 1, M]: one block per model, broadcast over the rows
    values = torch.stack([torch.as_tensor(m.eta.ect(), dtype=torch.float64) for m in dms]).to(dev)  # [B, M]
    out = kern.sample_paths(pp, torch.arange(rows.shape[0], device=dev), n_samples=n_samples, seed=seed)
    paths = out.paths  # [B, N, n_samples, L]
    track = torch.gather(values[:, None, None, :].expand(-1, paths.shape[1], paths.shape[2], -1), 3, paths.long())
    if single:
        paths, track = paths[0], track[0]
    if spans is None:
        return paths, track
    return ([paths[..., r : r + n, :, :length] for r, n, length in spans], [track[..., r : r + n, :, :length] for r, n, length in spans])


def tmrca_segments(path, values=None):
    """Run-length encoding of state paths on their device: ``path`` [L] or [N, L] (uint8 / integer tensor, 255 = past the
    row's end) -> ``(row, start, end, state)`` int64 tensors, one entry per maximal run of one state in one row (sites
    ``start .. end - 1``), rows in order; with ``values`` ([M], a value per state, e.g. ``dm.eta.ect()``) a fifth tensor
    ``values[state]``.  Runs of 255 are dropped."""
    p = torch.as_tensor(path)
    if p.ndim == 1:
        p = p[None]
    assert p.ndim == 2, "path: [L] or [N, L]"
    N, L = p.shape
    # one key per site that changes wherever the state or the row does
    key = p.reshape(-1).long() + 256 * torch.arange(N, device=p.device).repeat_interleave(L)
    uniq, counts = torch.unique_consecutive(key, return_counts=True)
    row, state = uniq // 256, uniq % 256
    end = torch.cumsum(counts, 0) - row * L
    start = end - counts
    keep = state != 255
    row, start, end, state = row[keep], start[keep], end[keep], state[keep]
    if values is None:
        return row, start, end, state
    v = torch.as_tensor(values, dtype=torch.float64, device=p.device)
    return row, start, end, state, v[state]


class SegmentSupport(NamedTuple):
    """What ``segment_support`` returns (float64 device tensors; lists with one tensor per contig for a list of contigs)."""

    logp: torch.Tensor  # [n]: log posterior probability of the segment's event under the equal-weight mixture of the models
    per_model: torch.Tensor  # [B, n]: the same under each model


def _near_sets(states, slack: int, M: int) -> np.ndarray:
    """bool [n, M]: per segment the states within ``slack`` of the segment's own"""
    st = np.asarray(states.cpu() if isinstance(states, torch.Tensor) else states).astype(np.int64).reshape(-1)
    assert ((st >= 0) & (st < M)).all(), f"states outside [0, {M})"
    assert int(slack) >= 0, "slack must be >= 0"
    return np.abs(np.arange(M)[None, :] - st[:, None]) <= int(slack)


def segment_support(dms, data, segments, *, states=None, slack: int = 1, t_max=None, t_min: float = 0.0, window_size: int = 100,
                    device=None, double_precision: bool = False) -> SegmentSupport:
    """How sure the data are of called segments: for every segment (row, start, end) the log posterior probability that the TMRCA
    state of EVERY window of the segment lies in the segment's set -- the question after ``viterbi_tmrca`` + ``tmrca_segments``,
    which ``tract_posterior`` answers on a fixed grid of bins and one set only.  Exact (``PSMCKernel.interval_tracts``), and a log:
    a segment of thousands of windows has a probability far below the float range.

    dms: one ``DemographicModel`` or the list ``fit()`` returns, evaluated per window as in ``posterior_tmrca``.
    data: int8 [N, L] het matrix of whole-contig rows, or a list of ``RawContig`` (or of int8 matrices) of different lengths (padded
        with missing windows; each row's own length bounds its segments).
    segments: what ``tmrca_segments`` returns -- (row, start, end, state, ...) with windows ``start .. end - 1`` of row ``row`` -- in
        any order, the segments of one row disjoint; for a list of contigs a list of such tables, rows counted per contig.
    states / slack: the set of segment j is the states within ``slack`` of ``states[j]`` (default: the table's fourth tensor, the
        segment's own state), the same for every model.
    t_max / t_min: instead, the set is per model the states whose whole interval lies in [t_min, t_max), exactly as
        ``tract_posterior`` decides it, the same for every segment.
    Returns ``SegmentSupport(logp, per_model)``: ``per_model`` float64 [B, n] and ``logp`` = logsumexp over the models - log B,
    the log posterior probability under the equal-weight mixture of the models (a probability given the data is linear in the
    mixture's components, see ``tract_posterior``).  For a list of contigs: lists with one tensor per contig.
    """
    if isinstance(dms, DemographicModel):
        dms = [dms]
    dms = list(dms)
    assert len(dms) > 0, "no model to decode under"
    M = dms[0].M
    assert all(dm.M == M for dm in dms), "all models must have the same number of states"
    if isinstance(data, (list, tuple)):
        for c in data:
            if isinstance(c, RawContig):
                c.get_data(window_size)  # (raises if the contig was built with another window size)
    rows, spans = _rows(data)
    lens = None
    host = lambda x: np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x).astype(np.int64).reshape(-1)  # noqa: E731
    if spans is None:
        tables = [segments]
        first_rows, n_rows = [0], [rows.shape[0]]
    else:
        tables = list(segments)
        assert len(tables) == len(spans), "segments: one table per contig"
        lens = np.concatenate([np.full(n, length, dtype=np.int64) for _, n, length in spans])
        first_rows, n_rows = [r for r, _, _ in spans], [n for _, n, _ in spans]
    counts = [host(t[0]).shape[0] for t in tables]
    for t, nr in zip(tables, n_rows):
        r = host(t[0])
        if r.size and (r.min() < 0 or r.max() >= nr):
            raise ValueError(f"segments: a row outside [0, {nr}) of its contig")
    row = np.concatenate([host(t[0]) + r0 for t, r0 in zip(tables, first_rows)])
    start, end = (np.concatenate([host(t[i]) for t in tables]) for i in (1, 2))
    if t_max is not None:
        assert states is None, "give states / slack or a time range, not both"
        masks = np.repeat(_range_sets(dms, t_min, t_max)[:, None, :], row.shape[0], axis=1)  # [B, n, M]
    else:
        if states is None:
            assert all(len(t) >= 4 for t in tables), "segments without a state column: give states or t_max"
            st = np.concatenate([host(t[3]) for t in tables])
        else:
            st = np.concatenate([host(x) for x in (states if spans is not None else [states])])
        assert st.shape[0] == row.shape[0], "states: one per segment"
        masks = _near_sets(st, slack, M)  # [n, M]
    kern = PSMCKernel(M, rows, double_precision=double_precision, device=device)
    per = [DemographicModel(eta=dm.eta, theta=float(dm.theta) * window_size, rho=float(dm.rho) * window_size) for dm in dms]
    pps = [PSMCParams.from_dm(dm) for dm in per]
    pp = PSMCParams(*(torch.stack([torch.as_tensor(getattr(p, f), dtype=torch.float64) for p in pps])[:, None]
                      for f in PSMCParams._fields))  # [B, 1, M]: one block per model, broadcast over the rows
    out = kern.interval_tracts(pp, torch.arange(rows.shape[0], device=kern.device), intervals=(row, start, end), masks=masks, lens=lens)
    per_model = out.logp  # [B, n] float64
    logp = torch.logsumexp(per_model, 0) - float(np.log(len(dms)))
    if spans is None:
        return SegmentSupport(logp, per_model)
    cuts = np.concatenate([[0], np.cumsum(counts)])
    return SegmentSupport([logp[a:b] for a, b in zip(cuts[:-1], cuts[1:])], [per_model[:, a:b] for a, b in zip(cuts[:-1], cuts[1:])])


class PathTracts(NamedTuple):
    """What ``path_tracts`` returns: int32 tensors on the device of the paths."""

    counts: torch.Tensor  # [..., n_samples, 4]: sites inside the set, tracts, longest tract, changes of state
    hist: torch.Tensor  # [..., n_samples, C]: tracts per length class, C = len(edges) + 1
    cover: torch.Tensor | None  # [..., nbin]: sites in tracts of at least min_len sites, summed over the samples, or None


def path_tracts(paths, in_set, *, edges=(), lens=None, min_len: int = 1, bin: int | None = None) -> PathTracts:
    """The tracts of stored state paths: what ``PSMCKernel.sample_tracts`` computes inside the kernel without storing a path, here
    from paths a caller holds (``PSMCKernel.sample_paths``, ``sample_tmrca``), in vectorised torch on the device of ``paths``.

    paths: integer tensor [..., n_samples, n] of states, the sites in order (a state of 255, past a Viterbi row's end, is
        outside every set).
    in_set: bool [M], or [B, M] with one row per entry of the FIRST dimension of ``paths``: the states that are inside.
    lens: integers broadcastable to ``paths.shape[:-2]``: how many of the n sites are the row's own (for paths of a kernel with
        ``overlap``: its ``lens`` minus the overlap); sites behind count for nothing.  None: all n.
    A tract is a maximal run of consecutive own sites whose state is inside; one that touches the first or the last own site
    is counted at its visible length.  ``counts`` [..., n_samples, 4]: own sites inside the set, number of tracts, length of the
    longest tract (0 if none), number of adjacent pairs of own sites whose states differ (whatever the set).  ``hist``
    [..., n_samples, C]: ``edges`` (strictly ascending lengths >= 1) cut the tract lengths into C = len(edges) + 1 classes, a
    tract of m sites falling in class #{e : edges[e] <= m}.  With ``bin`` given, ``cover`` [..., nbin], nbin = ceil(n / bin):
    per bin of ``bin`` sites the number of own sites that lie in a tract of at least ``min_len`` sites, summed over the
    samples.  Returns ``PathTracts(counts, hist, cover)``, int32."""
    p = torch.as_tensor(paths)
    assert p.ndim >= 2 and not p.dtype.is_floating_point, "paths: integer [..., n_samples, n]"
    dev = p.device
    edges = [int(e) for e in edges]
    assert all(e >= 1 for e in edges) and all(a < b for a, b in zip(edges, edges[1:])), "edges: strictly ascending lengths >= 1"
    assert int(min_len) >= 1 and (bin is None or int(bin) >= 1)
    lead, ns, n = p.shape[:-2], p.shape[-2], p.shape[-1]
    C = len(edges) + 1
    m = torch.as_tensor(in_set, device=dev).to(torch.bool)
    assert m.ndim in (1, 2) and m.shape[-1] <= 256, "in_set: bool [M] or [B, M]"
    table = torch.zeros(m.shape[:-1] + (256,), dtype=torch.bool, device=dev)  # (255 and every state beyond M: outside)
    table[..., : m.shape[-1]] = m
    z = p.long()
    if m.ndim == 1:
        inside = table[z]
    else:
        assert p.ndim >= 3 and m.shape[0] == p.shape[0], "in_set [B, M]: one row per entry of the first dimension of paths"
        inside = torch.gather(table.reshape((m.shape[0],) + (1,) * (p.ndim - 2) + (256,)).expand(p.shape[:-1] + (256,)), -1, z)
    own_len = torch.full(lead, n, dtype=torch.int64, device=dev) if lens is None else \
        torch.as_tensor(lens, device=dev).to(torch.int64).expand(lead).clamp(0, n)
    R = int(np.prod(lead, dtype=np.int64)) * ns
    own = torch.arange(n, device=dev)[None, :] < own_len.reshape(-1, 1).repeat_interleave(ns, 0)  # [R, n]
    z = z.reshape(R, n)
    inside = inside.reshape(R, n) & own
    pad = torch.zeros((R, 1), dtype=torch.bool, device=dev)
    first = inside & ~torch.cat([pad, inside[:, :-1]], 1)  # the first site of a tract
    last = inside & ~torch.cat([inside[:, 1:], pad], 1)  # its last site
    row, start = first.nonzero(as_tuple=True)  # (row-major order: the k-th start and the k-th end are one tract's)
    _, end = last.nonzero(as_tuple=True)
    length = end - start + 1
    counts = torch.zeros((R, 4), dtype=torch.int64, device=dev)
    counts[:, 0] = inside.sum(1)
    counts[:, 1] = first.sum(1)
    counts[:, 2] = torch.zeros(R, dtype=torch.int64, device=dev).scatter_reduce(0, row, length, "amax", include_self=True)
    counts[:, 3] = ((z[:, 1:] != z[:, :-1]) & own[:, 1:]).sum(1)
    cls = torch.bucketize(length, torch.tensor(edges, dtype=torch.int64, device=dev), right=True)  # = #{e : edges[e] <= length}
    hist = torch.zeros(R * C, dtype=torch.int64, device=dev).index_add_(0, row * C + cls, torch.ones_like(cls)).reshape(R, C)
    cover = None
    if bin is not None:
        bin = int(bin)
        nbin = (n + bin - 1) // bin
        keep = length >= int(min_len)
        d = torch.zeros(R * (n + 1), dtype=torch.int32, device=dev)  # +1 where a long tract starts, -1 behind its end
        one = torch.ones(int(keep.sum()), dtype=torch.int32, device=dev)
        d.index_add_(0, row[keep] * (n + 1) + start[keep], one)
        d.index_add_(0, row[keep] * (n + 1) + end[keep] + 1, -one)
        covered = torch.cumsum(d.reshape(R, n + 1)[:, :n], 1).reshape(-1, ns, n).sum(1)  # [rows, n]: samples whose long tract holds the site
        covered = torch.cat([covered, covered.new_zeros((covered.shape[0], nbin * bin - n))], 1)
        cover = covered.reshape(-1, nbin, bin).sum(2).to(torch.int32).reshape(lead + (nbin,))
    return PathTracts(counts.to(torch.int32).reshape(lead + (ns, 4)), hist.to(torch.int32).reshape(lead + (ns, C)), cover)


class TractSummary(NamedTuple):
    """Mean and central 95 % interval of a per-(model, sample) count, over models x samples with equal weight (float64)."""

    mean: torch.Tensor
    lo: torch.Tensor  # the 2.5 % quantile
    hi: torch.Tensor  # the 97.5 % quantile


class TractLengths(NamedTuple):
    """What ``tract_lengths`` returns: device tensors per row ([N, ...]) for a matrix; for a list of contigs ``in_long`` is a list
    with one tensor per contig, cut to the contig's own bins."""

    spectrum: TractSummary  # [N, C]: tracts per length class
    n_tracts: TractSummary  # [N]: number of tracts
    longest: TractSummary  # [N]: length of the longest tract, in windows
    inside: TractSummary  # [N]: windows inside the set
    in_long: object  # [N, nbin] float64: estimated P(the window lies in a tract of at least min_len windows | data)
    counts: torch.Tensor  # [B, N, n_samples, 4] int32: the raw counts per model and sample (``PSMCKernel.sample_tracts``)
    hist: torch.Tensor  # [B, N, n_samples, C] int32: the raw histograms


def _summary(x: torch.Tensor) -> TractSummary:
    """x [B, N, n_samples, ...] -> per row over models x samples"""
    x = x.to(torch.float64).transpose(0, 1)  # [N, B, n_samples, ...]
    x = x.reshape((x.shape[0], x.shape[1] * x.shape[2]) + tuple(x.shape[3:]))
    q = torch.quantile(x, torch.tensor([0.025, 0.975], dtype=torch.float64, device=x.device), dim=1)
    return TractSummary(x.mean(1), q[0], q[1])


def tract_lengths(dms, data, t_max, t_min: float = 0.0, *, n_samples: int = 64, seed: int = 0, edges=(10, 100, 1000), min_len: int = 100,
                  bin: int = 100, window_size: int = 100, in_set=None, device=None, double_precision: bool = False) -> TractLengths:
    """How many tracts every row of ``data`` has, how long they are, and which windows lie in a long one: the tracts of TMRCA in
    [t_min, t_max) (``t_max`` small: runs of homozygosity, IBD segments) in ``n_samples`` posterior paths per model, reduced on
    the GPU without a path being stored (``PSMCKernel.sample_tracts``).  None of this is additive over sites, so no exact sweep
    gives it; ``tract_posterior`` answers the other question, whether a fixed bin lies inside the range entirely.

    dms: one ``DemographicModel`` or the list ``fit()`` returns, evaluated per window as in ``posterior_tmrca``; the set of
        states of each model comes from [t_min, t_max) by ``tract_posterior``'s rule (a state is inside when its whole interval
        is).  ``in_set`` (bool [M] or [len(dms), M]) overrides it.
    data: int8 [N, L] het matrix of whole-contig rows, or a list of ``RawContig`` (or of int8 matrices) of different lengths:
        they are padded with missing windows and each row's own length goes to the kernel, which counts nothing behind it.
    edges: tract lengths in windows that cut the spectrum into len(edges) + 1 classes (a length equal to an edge goes up).
    min_len, bin: ``in_long`` is, per bin of ``bin`` windows, the share of (model, sample, own window of the bin) whose window
        lies in a tract of at least ``min_len`` windows.
    Returns ``TractLengths``; the summaries weigh models x samples equally.  The same ``seed`` gives the same numbers."""
    if isinstance(dms, DemographicModel):
        dms = [dms]
    dms = list(dms)
    assert len(dms) > 0, "no model to decode under"
    M = dms[0].M
    assert all(dm.M == M for dm in dms), "all models must have the same number of states"
    if in_set is None:
        assert float(t_min) < float(t_max), "the TMRCA range [t_min, t_max) is empty"
        w = np.empty((len(dms), M), dtype=bool)
        for i, dm in enumerate(dms):
            t = np.asarray(torch.as_tensor(dm.eta.t, dtype=torch.float64).cpu().numpy(), dtype=np.float64).reshape(M)
            lo, hi = t, np.append(t[1:], np.inf)
            w[i] = (lo >= float(t_min)) & (hi <= float(t_max))
    else:
        w = np.asarray(in_set.cpu() if isinstance(in_set, torch.Tensor) else in_set).astype(bool)
        assert w.shape in ((M,), (len(dms), M)), f"in_set: [{M}] or [{len(dms)}, {M}]"
    if isinstance(data, (list, tuple)):
        for c in data:
            if isinstance(c, RawContig):
                c.get_data(window_size)  # (raises if the contig was built with another window size)
    rows, spans = _rows(data)
    lens = None
    if spans is not None:
        lens = np.concatenate([np.full(n, length, dtype=np.int64) for _, n, length in spans])
    kern = PSMCKernel(M, rows, double_precision=double_precision, device=device)
    dev = kern.device
    per = [DemographicModel(eta=dm.eta, theta=float(dm.theta) * window_size, rho=float(dm.rho) * window_size) for dm in dms]
    pps = [PSMCParams.from_dm(dm) for dm in per]
    pp = PSMCParams(*(torch.stack([torch.as_tensor(getattr(p, f), dtype=torch.float64) for p in pps])[:, None]
                      for f in PSMCParams._fields))  # [B, 1, M]: one block per model, broadcast over the rows
    out = kern.sample_tracts(pp, torch.arange(rows.shape[0], device=dev), in_set=w, n_samples=n_samples, seed=seed, edges=edges,
                             lens=lens, min_len=min_len, bin=bin)
    own = torch.as_tensor(lens if lens is not None else np.full(rows.shape[0], rows.shape[1]), dtype=torch.int64, device=dev)
    sites = (own[:, None] - torch.arange(out.cover.shape[-1], dtype=torch.int64, device=dev)[None, :] * int(bin)).clamp_(0, int(bin))
    total = out.cover.sum(0, dtype=torch.int64).to(torch.float64)  # [N, nbin] over the models
    in_long = total / (len(dms) * int(n_samples) * sites.clamp(min=1)).to(torch.float64)
    if spans is not None:
        in_long = [in_long[r : r + n, : (length + int(bin) - 1) // int(bin)] for r, n, length in spans]
    c = out.counts
    return TractLengths(_summary(out.hist), _summary(c[..., 1]), _summary(c[..., 2]), _summary(c[..., 0]), in_long, c, out.hist)
