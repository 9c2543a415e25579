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

Both use inference semantics and leave the model, its engine's workspace and its optimizers alone.
"""
import collections
import ctypes

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
    mode = None
    if graphs is not None:
        if graphs != "sum":
            raise ValueError('score_recording: graphs must be None or "sum"')
        mode = gc_est_mode if gc_est_mode is not None else model.primary_gc_est_mode
        if mode not in GRAPH_MODES:
            raise ValueError("score_recording: graph traces are defined for the modes %s, got %s" % (GRAPH_MODES, mode))
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
