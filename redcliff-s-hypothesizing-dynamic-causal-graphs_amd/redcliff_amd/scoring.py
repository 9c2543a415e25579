"""Scoring whole recordings: factor scores and graph traces of every time step.

The reference answers "which factor is active at step i" with
``obtain_factor_score_weightings_across_recording`` / ``..._classifications_across_recording``
(general_utils/misc.py:57-81): one embedder call per step on a batch of one, each followed by a
copy to the host.  ``score_recording`` scores all steps of one or more recordings in one call:

* fused route (csrc/rc_score.hip, ``redcliff_score_recording``): a DGCNN model inside
  ``fused_supported()`` without wavelets whose shape the library accepts.  The sliding windows are
  never materialised; the optional graph trace is a second launch on the scores.
* fused cEmbedder route (csrc/rc_score_cemb.hip, ``redcliff_cemb_score_recording``), opt-in with
  ``REDCLIFF_CEMB_PATH=fused`` (cemb_engine.path_requested, read per call): a cEmbedder without
  wavelets, with one hidden layer and ``lag == embed_lag``, whose shape the library accepts.  The
  call is stateless: it packs a private copy of the embedder's parameters and touches no engine.
* chunked route, every other model: ``unfold`` and at most 512 windows per call through
  ``model.factor_score_embedder`` / ``model.GC``, with the embedder in eval mode for the duration.

All use inference semantics and leave the model, its engine's workspace and its optimizers alone.

``score_recordings`` scores a list of R models in one call: same-shape models inside the fused
route go through ``redcliff_score_recording_pack`` (the same kernels with the replica on a grid
axis: one prologue and one window-kernel launch for all R, bit for bit the models' own results);
any other list is scored model by model and stacked.  ``ReplicaPack.score_recording`` is the same
launch reading the pack's rows in place.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _native as nat
from .kernels import current_stream, ptr

CHUNK = 512  # windows per embedder call of the chunked route (the kernels' Bmax)
GRAPH_MODES = ("conditional_factor_exclusive", "conditional_factor_fixed_embedder")

RecordingScores = collections.namedtuple("RecordingScores", ["w", "logits", "graphs"])
RecordingScores.__doc__ = """w (Nrec, count, K); logits (Nrec, count, nsup) or None; graphs (Nrec, count, p, p, L') or None."""


def _score_dims(model):
    eng = model.engine()
    return eng.dims(1, eng.F)


def fused_available(model):
    """The fused kernel scores this model: inside fused_supported(), no wavelets, on the GPU, and
    the library accepts the shape (redcliff_score_recording_workspace_bytes > 0)."""
    if not model.fused_supported() or model.wavelet_level is not None:
        return False
    if not model.factor_score_embedder.dgcnn.dgcnn.A.is_cuda:
        return False
    d = _score_dims(model)
    return nat.lib().redcliff_score_recording_workspace_bytes(ctypes.byref(d)) > 0


def _window_args(model, X, start, count, stride):
    F = model.embed_lag
    if X.dim() == 2:
        X = X.unsqueeze(0)
    if X.dim() != 3 or X.shape[2] != model.num_series:
        raise ValueError("score_recording expects X of shape (T, %d) or (Nrec, T, %d), got %s" % (
            model.num_series, model.num_series, tuple(X.shape)))
    T = int(X.shape[1])
    start = F if start is None else int(start)
    stride = int(stride)
    if stride < 1:
        raise ValueError("score_recording: stride must be >= 1")
    if start < F:
        raise ValueError("score_recording: start=%d leaves no room for a window of embed_lag=%d steps" % (start, F))
    if count is None:
        count = (T - start) // stride + 1 if T >= start else 0
    count = int(count)
    if count < 0:
        raise ValueError("score_recording: count must be >= 0")
    if count > 0 and start + (count - 1) * stride > T:
        raise ValueError("score_recording: the last window ends at row %d, past T=%d" % (start + (count - 1) * stride, T))
    return X, start, count, stride


def _graph_mode(model, graphs, gc_est_mode):
    """The GC mode of the graph trace asked for with graphs / gc_est_mode; None without a trace."""
    if graphs is None:
        return None
    if graphs != "sum":
        raise ValueError('score_recording: graphs must be None or "sum"')
    mode = gc_est_mode if gc_est_mode is not None else model.primary_gc_est_mode
    if mode not in GRAPH_MODES:
        raise ValueError("score_recording: graph traces are defined for the modes %s, got %s" % (GRAPH_MODES, mode))
    return mode


def graph_tables(model, mode, ignore_lag):
    """(tab (K, p, p, L'), bias (p, p, L') | None) with
    sum(model.GC(mode, X=window, threshold=False, ignore_lag=ignore_lag)[0]) == bias + sum_k w_k tab[k]
    (...withStateSmoothing.py:481-498, :565-580), from the model's own _factor_gcs / _embedder_gc
    (DGCNN models) or its generic path's factor_gcs / fixed_embedder_gc (generic.py:472-498)."""
    K = model.num_factors_nK
    if not model.fused_supported():
        gp = model._generic()
        fg = torch.stack(gp.factor_gcs(False, ignore_lag))
        if mode == "conditional_factor_exclusive":
            return fg.contiguous(), None
        eg = gp.fixed_embedder_gc(False, ignore_lag, False)  # (p, p, 1) lag-free, else (p, p, embed_lag)
        if not ignore_lag:
            ls = min(model.gen_lag, model.embed_lag)
            fg = fg[..., -ls:]
            eg = eg[:, :, -ls:]
        return fg.contiguous(), (float(K) * eg).contiguous()
    fg = torch.stack(model._factor_gcs(False, ignore_lag))
    if mode == "conditional_factor_exclusive":
        return fg.contiguous(), None
    eg = model._embedder_gc(False, False)
    if not ignore_lag:
        ls = min(model.gen_lag, model.embed_lag)
        fg = fg[..., -ls:]
        eg = eg[:, :, -ls:]
    bias = (float(K) * eg).expand(fg.shape[1:])
    return fg.contiguous(), bias.contiguous()


def fused_score(model, X, start, count, stride, use_final_activation=True, tab=None, bias=None, out=None):
    """redcliff_score_recording on recordings X (Nrec, T, p) of a model inside fused_available().
    tab (K, ...) / bias: the graph trace's tables (graph_tables) or None.  out: optional
    (w, logits, graphs) contiguous device tensors to write into (tests place them inside guard
    buffers).  Returns (w, logits | None, graphs | None)."""
    eng = model.engine()
    eng.ensure_bound()
    dev = eng.device
    X = X.to(dev, torch.float32)
    if X.stride(2) != 1 or X.stride(1) != X.shape[2] or (X.shape[0] > 1 and X.stride(0) < 0):
        X = X.contiguous()  # rows of a recording must be contiguous; the recordings may be strided
    Nrec, T, _ = X.shape
    K, nsup = eng.K, eng.nsup
    d = _score_dims(model)
    L = nat.lib()
    nbytes = L.redcliff_score_recording_workspace_bytes(ctypes.byref(d))
    if nbytes == 0:
        nat.check(-2, "score_recording_workspace_bytes")
    ws = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
    ow, ol, og = out if out is not None else (None, None, None)
    w = ow if ow is not None else torch.empty(Nrec, count, K, device=dev, dtype=torch.float32)
    logits = None
    if nsup > 0:
        logits = ol if ol is not None else torch.empty(Nrec, count, nsup, device=dev, dtype=torch.float32)
    graphs = None
    a = nat.ScoreArgs()
    a.d = d
    a.emb, a.bn_rm, a.bn_rv = eng.emb.data_ptr(), eng.bn[0].data_ptr(), eng.bn[1].data_ptr()
    a.bn_eps = float(eng.dgcnn.BN1.eps)
    a.X, a.x_rstride = X.data_ptr(), int(X.stride(0)) if Nrec > 1 else 0
    a.Nrec, a.T = Nrec, T
    a.start, a.count, a.stride = start, count, stride
    a.use_final_activation = 1 if use_final_activation else 0
    a.w = w.data_ptr()
    a.logits = logits.data_ptr() if logits is not None else None
    if tab is not None:
        tab = tab.to(dev, torch.float32).contiguous()
        Q = tab[0].numel()
        graphs = og if og is not None else torch.empty((Nrec, count) + tuple(tab.shape[1:]), device=dev,
                                                       dtype=torch.float32)
        if bias is not None:
            bias = bias.to(dev, torch.float32).contiguous()
            assert bias.numel() == Q
            a.bias = bias.data_ptr()
        a.tab, a.graphs, a.Q = tab.data_ptr(), graphs.data_ptr(), Q
    for t in (w, logits, graphs):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.device == dev)
    if count == 0:  # nothing to launch (and empty tensors have no address to pass)
        return w, logits, graphs
    a.ws, a.ws_bytes = ws.data_ptr(), nbytes
    nat.check(L.redcliff_score_recording(ctypes.byref(a), current_stream()), "score_recording")
    return w, logits, graphs


def _cemb_dims(model):
    from . import cemb_engine as ce
    return ce.model_dims(model)


def cemb_config_supported(model):
    """The configuration half of cemb_fused_available (no device, no library call): a cEmbedder
    without wavelets, one embedder hidden layer, lag == embed_lag."""
    emb = model.factor_score_embedder
    if getattr(model, "factor_score_embedder_type", None) != "cEmbedder" or model.wavelet_level is not None:
        return False
    return emb.wavelet_level is None and len(emb.hidden) == 1 and emb.lag == model.embed_lag


def cemb_fused_available(model):
    """The fused cEmbedder kernel scores this model: a cEmbedder without wavelets, one embedder
    hidden layer, lag == embed_lag, parameters on the GPU, and the library accepts the shape
    (redcliff_cemb_score_supported > 0).  Only the embedder matters: num_sims, the forward mode and
    the factors play no part, so a model outside cembedder_fused_supported() may qualify."""
    if not cemb_config_supported(model):
        return False
    emb = model.factor_score_embedder
    if not emb.networks[0].layers[0].weight.is_cuda:
        return False
    d = _cemb_dims(model)
    return nat.lib().redcliff_cemb_score_supported(ctypes.byref(d), int(emb.hidden[0])) > 0


def cemb_packed(emb):
    """A private packed copy of a one-hidden-layer cEmbedder's parameters in the layout of
    cemb_engine.cemb_layout: We0[K][eh][p][F] | be0[K][eh] | We1[K][eh] | be1[K]."""
    nets = list(emb.networks)
    with torch.no_grad():
        return torch.cat([torch.stack([n.layers[0].weight for n in nets]).reshape(-1),
                          torch.stack([n.layers[0].bias for n in nets]).reshape(-1),
                          torch.stack([n.layers[1].weight for n in nets]).reshape(-1),
                          torch.stack([n.layers[1].bias for n in nets]).reshape(-1)]).float().contiguous()


def cemb_fused_score(model, X, start, count, stride, use_final_activation=True, tab=None, bias=None, out=None):
    """redcliff_cemb_score_recording on recordings X (Nrec, T, p) of a model inside
    cemb_fused_available(); arguments and result as fused_score.  Stateless: the kernel reads a
    packed copy of the module parameters made here; no engine, workspace or optimizer is touched."""
    emb = model.factor_score_embedder
    dev = emb.networks[0].layers[0].weight.device
    X = X.to(dev, torch.float32)
    if X.stride(2) != 1 or X.stride(1) != X.shape[2] or (X.shape[0] > 1 and X.stride(0) < 0):
        X = X.contiguous()  # rows of a recording must be contiguous; the recordings may be strided
    Nrec, T, _ = X.shape
    K, nsup = model.num_factors_nK, model.num_supervised_factors
    ow, ol, og = out if out is not None else (None, None, None)
    w = ow if ow is not None else torch.empty(Nrec, count, K, device=dev, dtype=torch.float32)
    logits = None
    if nsup > 0:
        logits = ol if ol is not None else torch.empty(Nrec, count, nsup, device=dev, dtype=torch.float32)
    graphs = None
    a = nat.CEmbScoreArgs()
    a.d = _cemb_dims(model)
    a.eh = int(emb.hidden[0])
    packed = cemb_packed(emb)
    a.emb = packed.data_ptr()
    a.X, a.x_rstride = X.data_ptr(), int(X.stride(0)) if Nrec > 1 else 0
    a.Nrec, a.T = Nrec, T
    a.start, a.count, a.stride = start, count, stride
    a.use_final_activation = 1 if use_final_activation else 0
    a.w = w.data_ptr()
    a.logits = logits.data_ptr() if logits is not None else None
    if tab is not None:
        tab = tab.to(dev, torch.float32).contiguous()
        Q = tab[0].numel()
        graphs = og if og is not None else torch.empty((Nrec, count) + tuple(tab.shape[1:]), device=dev,
                                                       dtype=torch.float32)
        if bias is not None:
            bias = bias.to(dev, torch.float32).contiguous()
            assert bias.numel() == Q
            a.bias = bias.data_ptr()
        a.tab, a.graphs, a.Q = tab.data_ptr(), graphs.data_ptr(), Q
    for t in (w, logits, graphs):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.device == dev)
    if count == 0:  # nothing to launch (and empty tensors have no address to pass)
        return w, logits, graphs
    nat.check(nat.lib().redcliff_cemb_score_recording(ctypes.byref(a), current_stream()), "cemb_score_recording")
    return w, logits, graphs


def _chunked_score(model, X, start, count, stride, use_final_activation, mode, ignore_lag):
    """unfold + at most CHUNK windows per call through the model's own embedder / GC."""
    emb = model.factor_score_embedder
    F = model.embed_lag
    dev = model._device()
    X = X.to(dev, torch.float32)
    Nrec = X.shape[0]
    time_major = model.factor_score_embedder_type != "DGCNN"  # the DGCNN embedder takes (B, p, F) nodes x features
    was_training = emb.training
    emb.eval()
    ws, ls, gs = [], [], []
    try:
        with torch.no_grad():
            for r in range(Nrec):
                win = X[r].unfold(0, F, 1)  # (T - F + 1, p, F): window i = rows [i, i + F)
                idx = torch.arange(count, device=dev) * stride + (start - F)
                wr, lr, gr = [], [], []
                for c0 in range(0, count, CHUNK):
                    xw = win[idx[c0:c0 + CHUNK]]
                    xt = xw.transpose(1, 2).contiguous()  # (B, F, p)
                    w, lg = emb(xt if time_major else xw.contiguous(), use_final_activation)
                    wr.append(w)
                    if lg is not None:
                        lr.append(lg)
                    if mode is not None:
                        gc = model.GC(mode, X=xt, threshold=False, ignore_lag=ignore_lag)
                        gr.append(torch.stack([sum(g) for g in gc]))
                K = model.num_factors_nK
                ws.append(torch.cat(wr) if wr else torch.empty(0, K, device=dev))
                if lr:
                    ls.append(torch.cat(lr))
                if mode is not None and gr:
                    gs.append(torch.cat(gr))
    finally:
        emb.train(was_training)
    w = torch.stack(ws)
    logits = torch.stack(ls) if ls else None
    graphs = torch.stack(gs) if gs else None
    return w, logits, graphs


def score_recording(model, X, start=None, count=None, stride=1, use_final_activation=True, graphs=None,
                    gc_est_mode=None, ignore_lag=True):
    """Factor scores (and, with graphs="sum", the summed conditional graph) of every scored step of
    recordings X (T, p) or (Nrec, T, p): step j uses rows [start + j*stride - F, start + j*stride)
    as a time-major window, F = embed_lag.  Defaults: start = F and every step that fits.
    Returns RecordingScores(w, logits, graphs)."""
    X, start, count, stride = _window_args(model, X, start, count, stride)
    mode = _graph_mode(model, graphs, gc_est_mode)
    if fused_available(model):
        with torch.no_grad():
            tab, bias = graph_tables(model, mode, ignore_lag) if mode is not None else (None, None)
            return RecordingScores(*fused_score(model, X, start, count, stride, use_final_activation, tab, bias))
    from . import cemb_engine
    if (getattr(model, "factor_score_embedder_type", None) == "cEmbedder" and cemb_engine.path_requested() == "fused"
            and cemb_fused_available(model)):
        with torch.no_grad():
            tab, bias = graph_tables(model, mode, ignore_lag) if mode is not None else (None, None)
            return RecordingScores(*cemb_fused_score(model, X, start, count, stride, use_final_activation, tab, bias))
    return RecordingScores(*_chunked_score(model, X, start, count, stride, use_final_activation, mode, ignore_lag))


# ----------------------------------------------------------------------------- many models, one launch
def _pack_window_args(model, X, R, start, count, stride):
    """The recordings of a call over R models: X (T, p) / (Nrec, T, p) shared by all of them, or
    one recording set per replica as a PerReplica list of R equal-shape tensors or an
    (R, Nrec, T, p) tensor.  Returns (X (Nrec, T, p) | (R, Nrec, T, p), per_replica, start, count,
    stride) under the rules of _window_args."""
    from .replicas import PerReplica
    if isinstance(X, PerReplica):
        if len(X) != R:
            raise ValueError("score_recording: PerReplica recordings: %d entries for %d replicas" % (len(X), R))
        parts = [_window_args(model, x, start, count, stride) for x in X]
        shapes = set(tuple(q[0].shape) for q in parts)
        if len(shapes) != 1:
            raise ValueError("score_recording: PerReplica recordings differ in shape: %s" % sorted(shapes))
        dev = parts[0][0].device
        return (torch.stack([q[0].to(dev, torch.float32) for q in parts]), True) + parts[0][1:]
    if X.dim() == 4:
        if X.shape[0] != R:
            raise ValueError("score_recording: per-replica recordings (R, Nrec, T, p) with R=%d for %d replicas" % (
                X.shape[0], R))
        return (X, True) + _window_args(model, X[0], start, count, stride)[1:]
    q = _window_args(model, X, start, count, stride)
    return (q[0], False) + q[1:]


def _active_indices(active, R):
    """Sorted replica indices of `active` (all R when None)."""
    if active is None:
        return list(range(R))
    idx = sorted(int(r) for r in active)
    if any(r < 0 or r >= R for r in idx) or len(set(idx)) != len(idx):
        raise ValueError("score_recording: active must list distinct replica indices < %d, got %s" % (R, list(active)))
    return idx


def pack_graph_tables(G, G0, A, mode, ignore_lag, ls):
    """graph_tables of R fused-route models at once, from their stacked group norms G (R, K, p, p, L)
    / G0 (R, K, p, p) and adjacencies A (R, p, p): (tab (R, K, p, p, L'), bias (R, p, p, L') | None).
    The same element-wise operations on the same values as graph_tables, so the same tables."""
    R, K, p = G0.shape[:3]
    fg = G if not ignore_lag else G0.reshape(R, K, p, p, 1)
    if mode == "conditional_factor_exclusive":
        return fg.contiguous(), None
    eg = A.transpose(1, 2).reshape(R, p, p, 1)
    if not ignore_lag:
        fg = fg[..., -ls:]
    bias = (float(K) * eg).expand((R,) + tuple(fg.shape[2:]))
    return fg.contiguous(), bias.contiguous()


def pack_launch(d, R, emb, emb_stride, bn_rm, bn_rv, bn_stride, bn_eps, X, per_replica, start, count, stride,
                use_final_activation=True, tab=None, bias=None, active=None, out=None):
    """redcliff_score_recording_pack: replica r's embedder block is emb's floats from r*emb_stride,
    its running statistics bn_rm / bn_rv's from r*bn_stride; X (Nrec, T, p) shared or, per_replica,
    (R, Nrec, T, p); tab (R, K, ...) / bias (R, ...) | None the replicas' graph tables; active: sorted
    replica indices or None (all).  out as fused_score.  Returns (w (Ra, Nrec, count, K),
    logits (Ra, Nrec, count, nsup) | None, graphs (Ra, Nrec, count, ...) | None), row i the i-th
    scored replica.  The workspace is private to the call."""
    dev = emb.device
    K, nsup = int(d.K), int(d.nsup)
    X = X.to(dev, torch.float32)
    lead = 1 if per_replica else 0
    if (X.stride(lead + 2) != 1 or X.stride(lead + 1) != X.shape[lead + 2]
            or any(X.shape[i] > 1 and X.stride(i) < 0 for i in range(lead + 1))):
        X = X.contiguous()  # rows of a recording must be contiguous; recordings and sets may be strided
    Nrec, T = int(X.shape[lead]), int(X.shape[lead + 1])
    idx = _active_indices(active, R)
    Ra = len(idx)
    ow, ol, og = out if out is not None else (None, None, None)
    w = ow if ow is not None else torch.empty(Ra, Nrec, count, K, device=dev, dtype=torch.float32)
    logits = None
    if nsup > 0:
        logits = ol if ol is not None else torch.empty(Ra, Nrec, count, nsup, device=dev, dtype=torch.float32)
    graphs = None
    a = nat.ScorePackArgs()
    a.d, a.R = d, R
    a.emb, a.emb_stride = emb.data_ptr(), int(emb_stride)
    a.bn_rm, a.bn_rv, a.bn_stride = bn_rm.data_ptr(), bn_rv.data_ptr(), int(bn_stride)
    a.bn_eps = float(bn_eps)
    a.X = X.data_ptr()
    a.x_rstride = int(X.stride(lead)) if Nrec > 1 else 0
    a.x_pstride = int(X.stride(0)) if per_replica and R > 1 else 0
    a.Nrec, a.T = Nrec, T
    a.start, a.count, a.stride = start, count, stride
    a.use_final_activation = 1 if use_final_activation else 0
    a.w = w.data_ptr()
    a.logits = logits.data_ptr() if logits is not None else None
    if tab is not None:
        tab = tab.to(dev, torch.float32).contiguous()
        assert tab.shape[0] == R and tab.shape[1] == K
        Q = tab[0, 0].numel()
        graphs = og if og is not None else torch.empty((Ra, Nrec, count) + tuple(tab.shape[2:]), device=dev,
                                                       dtype=torch.float32)
        if bias is not None:
            bias = bias.to(dev, torch.float32).contiguous()
            assert bias.numel() == R * Q
            a.bias = bias.data_ptr()
        a.tab, a.graphs, a.Q = tab.data_ptr(), graphs.data_ptr(), Q
    for t in (w, logits, graphs):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.device == dev)
    if count == 0 or Ra == 0:  # nothing to launch (and empty tensors have no address to pass)
        return w, logits, graphs
    if active is not None:
        act = np.ascontiguousarray(idx, dtype=np.int32)  # a host array: read before the call returns
        a.replicas, a.n_replicas = act.ctypes.data_as(ctypes.c_void_p), Ra
    L = nat.lib()
    nbytes = L.redcliff_score_recording_pack_workspace_bytes(ctypes.byref(d), R)
    if nbytes == 0:
        nat.check(-2, "score_recording_pack_workspace_bytes")
    ws = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
    a.ws, a.ws_bytes = ws.data_ptr(), nbytes
    nat.check(L.redcliff_score_recording_pack(ctypes.byref(a), current_stream()), "score_recording_pack")
    return w, logits, graphs


def _embedder_source(model, g, eng):
    """(packed embedder block, running mean, running var) of one model, read only: the engine's
    packed buffer when the embedder's parameters still alias it (the addresses of the embedder
    group alone are compared, not the whole model's), else the module's own tensors flattened in
    the packed layout (include/redcliff_hip.h).  The statistics are the module's buffers."""
    bn = g.BN1
    ptrs = eng.bound_ptrs
    if all(q.data_ptr() == ptrs[i] for i, q in enumerate(eng.group_params["A"])):
        return eng.emb, bn.running_mean, bn.running_var
    parts = [g.A] + [layer.weight for layer in g.layer1.gc1] + [bn.weight, bn.bias, g.fc1.linear.weight, g.fc1.linear.bias,
                                                                g.fc2.linear.weight, g.fc2.linear.bias]
    return torch.cat([t.detach().reshape(-1).float() for t in parts]), bn.running_mean, bn.running_var


def _pack_plan(models):
    """None unless one packed launch scores these models: each inside fused_available(), all of one
    embedder shape (p, K, nsup, F, n, H, M1, sigmoid, ecc), BatchNorm eps and device, at most 256 of
    them.  Else (dims, eps, [(embedder block, running mean, running var)]).  One pass over the
    models: a pack's host time is all spent before its first launch, with the GPU idle."""
    if not 1 <= len(models) <= 256:
        return None
    key0, srcs = None, []
    for m in models:
        if not m.fused_supported() or m.wavelet_level is not None:
            return None
        g = m.factor_score_embedder.dgcnn.dgcnn
        dev = g.A.device
        if dev.type != "cuda":
            return None
        eng = m._engine
        if eng is None or eng.device != dev:
            eng = m.engine()
        key = (eng.p, eng.K, eng.nsup, eng.F, eng.n, eng.H, eng.sig, eng.ecc, float(g.BN1.eps), dev)
        if key0 is None:
            key0 = key
        elif key != key0:
            return None
        srcs.append(_embedder_source(m, g, eng))
    d = _score_dims(models[0])
    if nat.lib().redcliff_score_recording_workspace_bytes(ctypes.byref(d)) == 0:  # one shape: one answer
        return None
    return d, key0[8], srcs


def pack_available(models):
    """One packed launch scores these models (see _pack_plan)."""
    return _pack_plan(list(models)) is not None


def _list_graph_tables(models, mode, ignore_lag):
    """(tab (R, K, p, p, L'), bias | None) of a list of fused-route models: one group-norm launch over
    a stacked copy of their factor blocks when those have one shape, graph_tables model by model
    otherwise.  Tables of different shapes cannot be stacked: ValueError."""
    engs = [m.engine() for m in models]
    e0 = engs[0]
    if all((e.L, e.h) == (e0.L, e0.h) for e in engs[1:]):
        for e in engs:
            # the norms read the layer-0 weights alone: every fourth parameter of the factor group
            # (kernels.factor_views).  While those alias the packed block it is current
            grp, ptrs, nA = e.group_params["B"], e.bound_ptrs, len(e.group_params["A"])
            if not all(grp[i].data_ptr() == ptrs[nA + i] for i in range(0, len(grp), 4)):
                e.ensure_bound()
        R = len(models)
        fac = torch.stack([e.fac for e in engs])
        d = nat.Dims(R=R, Bmax=1, T=e0.L, p=e0.p, L=e0.L, K=e0.K, h=e0.h, F=e0.L, n=1, H=1, M1=1, nsup=0,
                     use_sigmoid=0, sigmoid_ecc=0.0)
        G = torch.empty(R, e0.K, e0.p, e0.p, e0.L, device=e0.device, dtype=torch.float32)
        G0 = torch.empty(R, e0.K, e0.p, e0.p, device=e0.device, dtype=torch.float32)
        nat.check(nat.lib().redcliff_gc_norms(ctypes.byref(d), ptr(fac), fac.shape[1], ptr(G), ptr(G0), current_stream()),
                  "gc_norms (score_recordings)")
        A = torch.stack([e.dgcnn.A for e in engs]).float()
        return pack_graph_tables(G, G0, A, mode, ignore_lag, min(e0.L, e0.F))
    tabs = [graph_tables(m, mode, ignore_lag) for m in models]
    if len(set(tuple(t.shape) for t, _ in tabs)) != 1:
        raise ValueError("score_recordings: the models' graph tables differ in shape: %s" % sorted(
            set(tuple(t.shape) for t, _ in tabs)))
    return torch.stack([t for t, _ in tabs]), None if tabs[0][1] is None else torch.stack([b for _, b in tabs])


def fused_score_pack(models, X, per_replica, start, count, stride, use_final_activation=True, tab=None, bias=None,
                     active=None, out=None, plan=None):
    """pack_launch on a list of models inside pack_available(): stateless -- the kernels read a
    private [R][PA] copy of the embedder blocks and a [2][R][F] copy of the running statistics made
    here; no engine, workspace, optimizer or module state is touched."""
    d, eps, srcs = plan if plan is not None else _pack_plan(models)
    emb = torch.stack([q[0] for q in srcs])
    bn = torch.stack([torch.stack([q[1] for q in srcs]), torch.stack([q[2] for q in srcs])]).float()  # [2][R][F]
    return pack_launch(d, len(models), emb, emb.shape[1], bn[0], bn[1], bn.shape[2], eps, X, per_replica, start, count,
                       stride, use_final_activation, tab, bias, active, out)


def _stack_scores(parts, what="score_recordings"):
    """RecordingScores of a list of per-model results with a leading replica axis."""
    out = []
    for field in range(3):
        vals = [q[field] for q in parts]
        if all(v is None for v in vals):
            out.append(None)
            continue
        if any(v is None for v in vals) or len(set(tuple(v.shape) for v in vals)) != 1:
            raise ValueError("%s: the models' %s cannot be stacked: shapes %s" % (
                what, RecordingScores._fields[field], [None if v is None else tuple(v.shape) for v in vals]))
        out.append(torch.stack(vals))
    return RecordingScores(*out)


def score_recordings(models, X, start=None, count=None, stride=1, use_final_activation=True, graphs=None,
                     gc_est_mode=None, ignore_lag=True):
    """score_recording for a list of R models in one call: RecordingScores with a leading replica
    axis, w (R, Nrec, count, K), logits (R, Nrec, count, nsup) | None, graphs (R, Nrec, count, p, p, L')
    | None, row r bit for bit what models[r].score_recording gives.  X: (T, p) or (Nrec, T, p) shared
    by all models, or one recording set per model as a PerReplica list of R equal-shape tensors or an
    (R, Nrec, T, p) tensor.  Stateless: any list of models (checkpointed fold models, grid points),
    no optimizers or pack needed.

    Models inside pack_available() are scored by one packed launch chain (csrc/rc_score.hip,
    redcliff_score_recording_pack: one window-kernel launch for all R).  Models whose results could
    not be stacked (different K, nsup or graph-table shape) raise ValueError; every other list (a
    cEmbedder, num_sims = 2, wavelets, mixed shapes ...) is scored model by model and stacked."""
    models = list(models)
    R = len(models)
    if R < 1:
        raise ValueError("score_recordings: empty list of models")
    m0 = models[0]
    for key in ("num_factors_nK", "num_supervised_factors", "num_series"):
        vals = [getattr(m, key) for m in models]
        if len(set(vals)) != 1:
            raise ValueError("score_recordings: the models differ in %s (%s): their results cannot be stacked" % (key, vals))
    modes = [_graph_mode(m, graphs, gc_est_mode) for m in models]
    Xn, per_replica, s0, c0, st = _pack_window_args(m0, X, R, start, count, stride)
    same_window = len(set(m.embed_lag for m in models)) == 1
    plan = _pack_plan(models) if same_window and len(set(modes)) == 1 else None
    if plan is not None:
        mode = modes[0]
        with torch.no_grad():
            tab, bias = _list_graph_tables(models, mode, ignore_lag) if mode is not None else (None, None)
            return RecordingScores(*fused_score_pack(models, Xn, per_replica, s0, c0, st, use_final_activation, tab, bias,
                                                     plan=plan))
    parts = [m.score_recording(Xn[r] if per_replica else Xn, start, count, stride, use_final_activation, graphs,
                               gc_est_mode, ignore_lag) for r, m in enumerate(models)]
    return _stack_scores(parts)
