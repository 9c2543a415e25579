"""Host side of the fused engines (redcliff_amd.engine.PackedEngine and its two subclasses, the
DGCNN FitEngine and the cEmbedder CEmbEngine) on CPU models: parameter packing, optimizer binding,
re-binding, and the class layout.  Needs no GPU and no library: nothing here launches a kernel."""
import pytest
import torch

from test_cemb_host import cpu_model as cemb_model

DGCNN_ONLY = ("attach_pack", "plan_steps", "bn_stats", "forward_outputs", "embed_raw", "status_view",
              "_run_values_grouped")


def dgcnn_model():
    """smoke()'s shape: p=6 L=3 K=3 h=8 F=5 n=3 H=7."""
    import redcliff_amd
    from oracle.redcliff_oracle import reference_coeffs
    p, L, K, h, F, n, H = 6, 3, 3, 8, 5, 3, 7
    eargs = [("num_features_per_node", F), ("num_graph_conv_layers", n), ("num_hidden_nodes", H),
             ("sigmoid_eccentricity_coeff", 10.0)]
    torch.manual_seed(0)
    return redcliff_amd.REDCLIFF_S_CMLP_withStateSmoothing(
        p, L, [h], F, [0], L, 1, K, K, reference_coeffs(K, p), False, "DGCNN", eargs,
        "conditional_factor_fixed_embedder", "apply_factor_weights_after_sim_completion", num_sims=1,
        training_mode="pretrain_embedder_then_acclimate_factors_then_combined", num_pretrain_epochs=1,
        num_acclimation_epochs=1).float()


def engine_of(kind, m):
    from redcliff_amd.cemb_engine import CEmbEngine
    from redcliff_amd.engine import FitEngine
    return FitEngine(m) if kind == "dgcnn" else CEmbEngine(m)


@pytest.fixture(params=["dgcnn", "cemb"])
def kind(request):
    return request.param


def fresh(kind):
    return dgcnn_model() if kind == "dgcnn" else cemb_model()


def inside(t, buf):
    """Offset (elements) of tensor t in the flat buffer buf; asserts t lies wholly inside it."""
    off = t.data_ptr() - buf.data_ptr()
    assert off % 4 == 0 and 0 <= off // 4 and off // 4 + t.numel() <= buf.numel()
    return off // 4


def groups(m, eng):
    return (("A", m.gen_model[0], eng.emb), ("B", m.gen_model[1], eng.fac))


def test_parameters_are_views_that_tile_the_buffers(kind):
    m = fresh(kind)
    before = dict((k, v.detach().clone()) for k, v in m.state_dict().items())
    eng = engine_of(kind, m)
    for g, mod, buf in groups(m, eng):
        prms = list(mod.parameters())
        spans = sorted((inside(p, buf), p.numel()) for p in prms)
        assert sum(n for _, n in spans) == buf.numel()
        assert all(a + n == b for (a, n), (b, _) in zip(spans, spans[1:])) and spans[0][0] == 0
        assert [id(p) for p in eng._group_params(g)] == [id(p) for p in prms]
        # a NaN-filled buffer has no NaN left after the parameters are copied in
        vals = [p.detach().clone() for p in prms]
        with torch.no_grad():
            buf.fill_(float("nan"))
            for p, v in zip(prms, vals):
                p.copy_(v)
        assert not torch.isnan(buf).any()
    after = m.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k


def stepped_adam(mod, seed):
    """An Adam over mod's parameters after one torch step on seeded gradients."""
    opt = torch.optim.Adam(mod.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-4, weight_decay=1e-4)
    gen = torch.Generator().manual_seed(seed)
    for p in mod.parameters():
        p.grad = torch.randn(p.shape, generator=gen)
    opt.step()
    opt.zero_grad(set_to_none=True)
    return opt


def test_bind_optimizer_takes_over_a_torch_stepped_adam(kind):
    m = fresh(kind)
    opts = {"A": stepped_adam(m.gen_model[0], 1), "B": stepped_adam(m.gen_model[1], 2)}
    eng = engine_of(kind, m)
    for g, mod, buf in groups(m, eng):
        opt = opts[g]
        want = dict((id(p), (opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()))
                    for p in mod.parameters())
        st = eng.bind_optimizer(g, opt)
        assert st["t"] == 1 and float(st["step"]) == 1.0
        assert st["m"].shape == buf.shape and st["v"].shape == buf.shape
        steps = set()
        for p in mod.parameters():
            off, n = inside(p, buf), p.numel()
            ea, eas = want[id(p)]
            assert torch.equal(st["m"][off:off + n], ea.reshape(-1))
            assert torch.equal(st["v"][off:off + n], eas.reshape(-1))
            s = opt.state[p]
            assert s["exp_avg"].shape == p.shape and inside(s["exp_avg"], st["m"]) == off
            assert s["exp_avg_sq"].shape == p.shape and inside(s["exp_avg_sq"], st["v"]) == off
            steps.add(id(s["step"]))
        assert steps == {id(st["step"])}  # one shared step tensor
        assert eng.bind_optimizer(g, opt) is st


def test_ensure_bound_picks_up_a_repointed_parameter(kind):
    m = fresh(kind)
    eng = engine_of(kind, m)
    for g, mod, buf in groups(m, eng):
        prm = list(mod.parameters())[-1]
        off = inside(prm, buf)
        new = torch.full(prm.shape, 0.25 if g == "A" else -0.5)
        prm.data = new
        assert prm.data_ptr() == new.data_ptr()
        eng.ensure_bound()
        assert inside(prm, buf) == off
        assert torch.equal(buf[off:off + prm.numel()], new.reshape(-1)) and torch.equal(prm.detach(), new)


def test_bind_optimizer_refusals(kind):
    m = fresh(kind)
    eng = engine_of(kind, m)
    mine = list(m.gen_model[0].parameters())
    with pytest.raises(NotImplementedError):
        eng.bind_optimizer("A", torch.optim.SGD(mine, lr=0.1))
    with pytest.raises(NotImplementedError):
        eng.bind_optimizer("A", torch.optim.Adam([{"params": mine[:1]}, {"params": mine[1:]}], lr=0.1))
    with pytest.raises(NotImplementedError):
        eng.bind_optimizer("A", torch.optim.Adam(mine, lr=0.1, amsgrad=True))
    with pytest.raises(ValueError):
        eng.bind_optimizer("A", torch.optim.Adam(m.gen_model[1].parameters(), lr=0.1))
    with pytest.raises(ValueError):
        eng.bind_optimizer("B", torch.optim.Adam(mine, lr=0.1))
    assert eng.opt == {"A": None, "B": None}


def test_cemb_engine_has_no_dgcnn_only_method():
    from redcliff_amd.engine import FitEngine
    ceng = engine_of("cemb", cemb_model())
    assert [n for n in DGCNN_ONLY if hasattr(ceng, n)] == []
    assert [n for n in DGCNN_ONLY if not hasattr(FitEngine, n)] == []


def test_engine_classes_meet_only_at_the_shared_base():
    from redcliff_amd.cemb_engine import CEmbEngine
    from redcliff_amd.engine import FitEngine, PackedEngine
    assert set(FitEngine.__mro__) & set(CEmbEngine.__mro__) == {PackedEngine, object}
    assert FitEngine.__mro__[1] is PackedEngine and CEmbEngine.__mro__[1] is PackedEngine
