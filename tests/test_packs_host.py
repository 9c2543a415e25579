"""CPU checks of what the baselines' fused routes share on the host (redcliff_amd.packs, and the native-call
helpers of redcliff_amd._native): packing, the binding of a torch.optim.Adam's state to the pack's rows, the
replica hyper-parameter records and their cache, the step counters, the replica list, the route switch and
the model-side slot.  A minimal pack of two parameters on CPU tensors; no kernel is launched."""
import copy
import ctypes
import io

import numpy as np
import pytest
import torch
import torch.nn as nn

from redcliff_amd import _native as nat
from redcliff_amd import packs

LAYOUT = [("w", 0, (3, 2)), ("b", 6, (2,))]
SIZE, R = 8, 2
C_ADJ = 0.25


class TinyPack(packs.AdamPack):
    def __init__(self, models):
        self.allocate(models, SIZE, torch.device("cpu"))
        for r, mod in enumerate(self.models):
            prms = [mod.w, mod.b]
            packs.pack_by_layout(self.par[r], prms, LAYOUT)
            self.adopt(r, prms)

    def replica_terms(self, r):
        return {"c_adj": C_ADJ * (r + 1)}


class BiasOnlyPack(TinyPack):
    def stepped_parameters(self, r):
        return self.params[r][1:]


class Tiny(packs.PackSlot, nn.Module):
    _slot_key, _pack_class = "_tiny_slot", TinyPack

    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w = nn.Parameter(torch.randn(3, 2, generator=g))
        self.b = nn.Parameter(torch.randn(2, generator=g))


def torch_step(model, opt, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(5, 3, generator=g)
    opt.zero_grad()
    ((x @ model.w + model.b) ** 2).sum().backward()
    opt.step()


def inside(view, row, off):
    return view.data_ptr() == row.data_ptr() + 4 * off


def test_packing_keeps_values_and_tracks_the_pointers():
    models = [Tiny(1), Tiny(2)]
    want = [(m.w.detach().clone(), m.b.detach().clone()) for m in models]
    pack = TinyPack(models)
    assert pack.par.shape == (R, SIZE) and pack.np_ == SIZE
    for r, m in enumerate(models):
        for prm, (_, off, shp), w in zip((m.w, m.b), LAYOUT, want[r]):
            assert inside(prm, pack.par[r], off) and tuple(prm.shape) == shp
            assert torch.equal(prm.detach(), w)
            assert torch.equal(pack.par[r, off:off + prm.numel()].view(shp), w)
        assert pack.bound(r) and m.__dict__["_tiny_slot"] == (pack, r)
    models[1].b.data = models[1].b.data.clone()
    assert pack.bound(0) and not pack.bound(1)


@pytest.mark.parametrize("r", [0, 1])
def test_fresh_adam_state_becomes_views_of_the_rows(r):
    models = [Tiny(1), Tiny(2)]
    pack = TinyPack(models)
    m = models[r]
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    st = pack.bind_optimizer(r, opt)
    assert st["t"] == 0 and pack.opt[r] is st
    for prm, (_, off, _) in zip((m.w, m.b), LAYOUT):
        s = opt.state[prm]
        assert inside(s["exp_avg"], pack.m[r], off) and inside(s["exp_avg_sq"], pack.v[r], off)
        assert s["exp_avg"].shape == prm.shape and float(s["step"]) == 0.0
    assert not pack.m.any() and not pack.v.any()
    torch_step(m, opt, 3)
    assert pack.m[r].abs().min() > 0 and pack.v[r].abs().min() > 0 and not pack.m[1 - r].any()


@pytest.mark.parametrize("r", [0, 1])
def test_resume_from_a_stepped_adam_and_rebinding(r):
    models = [Tiny(1), Tiny(2)]
    m = models[r]
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    for k in range(3):
        torch_step(m, opt, 10 + k)
    was = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in (m.w, m.b)]
    pack = TinyPack(models)
    st = pack.bind_optimizer(r, opt)
    assert st["t"] == 3
    for (_, off, shp), (ea, eas) in zip(LAYOUT, was):
        n = int(np.prod(shp))
        assert torch.equal(pack.m[r, off:off + n].view(shp), ea) and torch.equal(pack.v[r, off:off + n].view(shp), eas)
    assert not pack.m[1 - r].any() and not pack.v[1 - r].any()
    for k in range(2):
        torch_step(m, opt, 20 + k)
    assert pack.bind_optimizer(r, opt) is st and st["t"] == 5
    assert all(float(opt.state[p]["step"]) == 5.0 for p in (m.w, m.b))


def test_stepped_parameters_hook_leaves_the_others_without_state():
    models = [Tiny(1), Tiny(2)]
    pack = BiasOnlyPack(models)
    m = models[0]
    opt = torch.optim.Adam([m.b], lr=1e-2)
    pack.bind_optimizer(0, opt)
    assert m.w not in opt.state and m.b in opt.state
    torch_step(m, opt, 4)
    assert not pack.m[0, :6].any() and not pack.v[0, :6].any() and pack.m[0, 6:].abs().min() > 0


def expected_hyper(pack, t_base, reps, adams):
    want = (nat.ReplicaHyper * R)()
    for r in range(R):
        h = want[r]
        h.c_adj = C_ADJ * (r + 1)
        h.bn_eps, h.bn_momentum = 1e-5, 0.1
        h.A = nat.adam_hyper(0.0, (0.9, 0.999), 1e-8, 0.0)
        h.B = nat.adam_hyper(*adams[r])
        h.B.t_offset = (pack.opt[r]["t"] - t_base) if r in reps else 0
    return bytes(want)


def test_hyper_records_and_their_cache():
    models = [Tiny(1), Tiny(2)]
    pack = TinyPack(models)
    opts = [torch.optim.Adam(models[0].parameters(), lr=1e-2, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.5),
            torch.optim.Adam(models[1].parameters(), lr=3e-3)]
    torch_step(models[1], opts[1], 5)
    torch_step(models[1], opts[1], 6)
    for r in range(R):
        pack.bind_optimizer(r, opts[r])
    assert (pack.opt[0]["t"], pack.opt[1]["t"]) == (0, 2)
    adams = [(1e-2, (0.8, 0.95), 1e-6, 0.5), (3e-3, (0.9, 0.999), 1e-8, 0.0)]
    both = pack.hyper(0, [0, 1])
    assert both.dtype == torch.uint8 and bytes(both.numpy()) == expected_hyper(pack, 0, [0, 1], adams)
    assert pack.hyper(0, [0, 1]) is both
    one = pack.hyper(2, [1])
    assert one is not both and bytes(one.numpy()) == expected_hyper(pack, 2, [1], adams)
    assert pack.hyper(2, [1]) is one
    opts[0].param_groups[0]["lr"] = 5e-3
    changed = pack.hyper(2, [1])
    adams[0] = (5e-3,) + adams[0][1:]
    assert bytes(changed.numpy()) != bytes(one.numpy()) and bytes(changed.numpy()) == expected_hyper(pack, 2, [1], adams)


def test_reps_and_advance_move_the_listed_rows_only():
    models = [Tiny(1), Tiny(2)]
    pack = TinyPack(models)
    opts = [torch.optim.Adam(m.parameters(), lr=1e-2) for m in models]
    for r in range(R):
        pack.bind_optimizer(r, opts[r])
    assert pack.reps(None) == [0, 1] and pack.reps((1,)) == [1]
    pack.advance([1], 7)
    assert pack.opt[0]["t"] == 0 and pack.opt[1]["t"] == 7
    assert all(float(opts[0].state[p]["step"]) == 0.0 for p in models[0].parameters())
    assert all(float(opts[1].state[p]["step"]) == 7.0 for p in models[1].parameters())
    pack.advance(pack.reps(None), 2)
    assert pack.opt[0]["t"] == 2 and pack.opt[1]["t"] == 9 and float(opts[1].state[models[1].b]["step"]) == 9.0
    with pytest.raises(RuntimeError):
        TinyPack([Tiny(3)]).require_optimizers([0])


def test_workspace_grows_only():
    pack = TinyPack([Tiny(1)])
    ws = pack.workspace_of(16)
    assert ws.numel() == 16 and pack.workspace_of(8) is ws and pack.workspace_of(16) is ws
    assert pack.workspace_of(17).numel() == 17


def test_replica_list_and_ptr():
    a = nat.NavarArgs()
    assert nat.replica_list(a, None) is None and a.n_replicas == 0 and not a.replicas
    keep = nat.replica_list(a, [4, 0, 2])
    assert a.n_replicas == 3
    got = ctypes.cast(a.replicas, ctypes.POINTER(ctypes.c_int32))
    assert [got[i] for i in range(3)] == [4, 0, 2] and list(keep) == [4, 0, 2]
    b = nat.FMArgs()
    keep = nat.replica_list(b, [])
    assert b.n_replicas == 0 and b.replicas and len(keep) == 1
    t = torch.zeros(3)
    assert nat.ptr(None) is None and nat.ptr(t) == t.data_ptr()
    s = ctypes.c_void_p(5)
    assert nat.stream_or_current(s) is s


def test_route_from_env(monkeypatch):
    var = "REDCLIFF_PACKS_TEST_PATH"
    monkeypatch.delenv(var, raising=False)
    assert packs.route_from_env(var) == "fused" and packs.route_from_env(var, "generic") == "generic"
    monkeypatch.setenv(var, "")
    assert packs.route_from_env(var) == "fused"
    monkeypatch.setenv(var, "generic")
    assert packs.route_from_env(var) == "generic"
    monkeypatch.setenv(var, "eager")
    with pytest.raises(ValueError, match=var):
        packs.route_from_env(var)


def test_copies_and_pickles_drop_the_slot():
    models = [Tiny(1), Tiny(2)]
    pack = TinyPack(models)
    m = models[1]
    m.__dict__["_cache"] = "kept"
    dup = copy.deepcopy(m)
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=False)
    for c in (dup, loaded):
        assert "_tiny_slot" not in c.__dict__ and c.__dict__["_cache"] == "kept"
        assert torch.equal(c.w, m.w) and torch.equal(c.b, m.b)
        own, row = c._slot()
        assert own is not pack and own.R == 1 and row == 0 and own.bound(0) and c._slot() == (own, 0)
    assert m._slot() == (pack, 1)
