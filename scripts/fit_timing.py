"""The timing protocol the baselines' fit scripts share (fm_fit.py, lstm_fm_fit.py, navar_fit.py,
navar_lstm_fit.py, dgcnn_fit.py, dcsfa_fit.py): a run between two HIP events, and the summary of its samples."""
import statistics
import time

import torch


def event_ms(fn):
    """(ms between two HIP events around fn, host ms fn took to enqueue its work)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    b.record()
    b.synchronize()
    return a.elapsed_time(b), host


def summary(s, epochs, steps):
    med = statistics.median(s)
    return {"median_ms": med, "min_ms": min(s), "max_ms": max(s), "spread_ms": max(s) - min(s), "samples_ms": s,
            "us_per_epoch": {"median": 1e3 * med / epochs, "min": 1e3 * min(s) / epochs, "max": 1e3 * max(s) / epochs},
            "us_per_step": {"median": 1e3 * med / (epochs * steps), "min": 1e3 * min(s) / (epochs * steps),
                            "max": 1e3 * max(s) / (epochs * steps)}}
