"""Node-output dropout of the layer stack (-m gpu): the kernels of csrc/gnm_dropout.hip bit for bit against the numpy restatement
of the mask function (tests/dropout_reference.py, itself checked against the published Philox vectors in test_dropout_cpu.py), and
the model / stack routes that use them -- against an fp64 torch restatement with the exported masks multiplied in, across the
backward schedules, the recomputing modes, the seed / step bookkeeping, and with the feature switched off.

Tolerances of the model cases: those of the p = 0 cases (helpers.assert_parity for the logits, 1e-5 on the loss, helpers.GRAD_L2
rel-L2 per gradient tensor or the absolute floor max(GRAD_ABS_FLOOR, 1e-6 x the largest gradient norm) for the analytically zero
ones).  Dropout adds one exact multiply by a power-of-two-free constant that both sides share, so nothing is widened.  There is no
branch-exact clause here: on the 64-node fixtures no relu decision sits within fp32 round-off of its kink."""
import os

import numpy as np
import pytest
import torch

import dropout_reference as ref
from helpers import GOLDEN, GRAD_ABS_FLOOR, GRAD_L2, assert_parity, rel_l2, sd_to_torch
from oracle import gatedgcn_oracle as orc

pytestmark = pytest.mark.gpu

SEED = 0x5EEDC0DE12345678


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _ids(kind, N, rng):
    if kind == "identity":
        return None, np.arange(N, dtype=np.int64)
    ids = rng.permutation(N).astype(np.int32)
    return ids, ids.astype(np.int64)


def _dev_mask(N, H, p, seed, step, layer, ids, dev):
    from gnnome_assembly_amd import engine
    t = None if ids is None else torch.from_numpy(ids).to(dev)
    m = engine.dropout_mask(N, H, (p, seed, step), layer, dev, t)
    assert m.dtype == torch.uint8 and tuple(m.shape) == (N, H)
    return m.cpu().numpy()


# ---- 1. mask bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [32, 100, 256])
def test_mask_bits(H):
    dev = _dev()
    rng = np.random.default_rng(H)
    for N in (1, 63, 1025):
        for p in (0.1, 0.5):
            for kind in ("identity", "shuffled"):
                ids, v = _ids(kind, N, rng)
                step, layer = int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 16))
                got = _dev_mask(N, H, p, SEED, step, layer, ids, dev)
                want = ref.keep_mask(v, H, p, SEED, step, layer)
                assert set(np.unique(got)) <= {0, 1}
                assert np.array_equal(got.astype(bool), want), (N, H, p, kind, int((got.astype(bool) != want).sum()))


def test_mask_bits_past_2_to_32_elements():
    """Four rows whose node ids lie just below 2^31 at H = 256: the element index v H + c passes 2^32 (q needs its high word)
    with nothing large allocated."""
    dev = _dev()
    ids = np.arange(2 ** 31 - 4, 2 ** 31, dtype=np.int64).astype(np.int32)
    got = _dev_mask(4, 256, 0.5, SEED, 3, 1, ids, dev)
    want = ref.keep_mask(ids.astype(np.int64), 256, 0.5, SEED, 3, 1)
    assert np.array_equal(got.astype(bool), want)
    assert not np.array_equal(want, ref.keep_mask(ids.astype(np.int64) & 0xFFFFFF, 256, 0.5, SEED, 3, 1))    # the high word matters


def test_mask_does_not_depend_on_the_occupancy_cap():
    from gnnome_assembly_amd import _lib
    dev = _dev()
    lib = _lib.load()
    N, H = 1025, 256
    try:
        masks = []
        for cap in (1, 0):          # one workgroup per CU, then no cap: two grids
            _lib.check(lib.gnm_set_occupancy_cap(cap), "gnm_set_occupancy_cap")
            masks.append(_dev_mask(N, H, 0.5, SEED, 9, 2, None, dev))
    finally:
        _lib.check(lib.gnm_set_occupancy_cap(0), "gnm_set_occupancy_cap")
    assert np.array_equal(masks[0], masks[1])
    assert np.array_equal(masks[0].astype(bool), ref.keep_mask(np.arange(N), H, 0.5, SEED, 9, 2))


# ---- 2. apply bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,ld", [(32, 32), (100, 128), (256, 256), (30, 32)])
def test_apply_bits(H, ld):
    """y = where(mask, x float32(1 / (1 - p)), +0) bit for bit, in place and out of place; the columns H .. ld-1 are left alone.
    (30, 32): a width that is no multiple of 4 takes the element-by-element kernel."""
    from gnnome_assembly_amd import engine
    dev = _dev()
    rng = np.random.default_rng(H + ld)
    for N in (1, 63, 1025):
        for p in (0.1, 0.5):
            for kind in ("identity", "shuffled"):
                ids, v = _ids(kind, N, rng)
                x = rng.standard_normal((N, ld)).astype(np.float32)
                x[0, 0] = -0.0
                step, layer = int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 16))
                keep = ref.keep_mask(v, H, p, SEED, step, layer)
                want = x.copy()
                want[:, :H] = ref.apply(x[:, :H], keep, p)
                t = None if ids is None else torch.from_numpy(ids).to(dev)
                xd = torch.from_numpy(x).to(dev)
                out = torch.full_like(xd, 7.0)
                y = engine.node_dropout(xd, (p, SEED, step), layer, H, t, out=out)
                assert y is out and torch.equal(xd.cpu(), torch.from_numpy(x))          # out of place: x untouched
                got = out.cpu().numpy()
                assert np.array_equal(got[:, :H].view(np.int32), want[:, :H].view(np.int32)), (N, H, p, kind)
                assert np.all(got[:, H:] == 7.0)
                y = engine.node_dropout(xd, (p, SEED, step), layer, H, t)               # in place
                assert y is xd
                assert np.array_equal(xd.cpu().numpy().view(np.int32), want.view(np.int32)), (N, H, p, kind)


# ---- 3. keep rate -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate(p):
    """The kept fraction of N H = 4096 x 128 independent draws is within 5 sigma of 1 - p, sigma = sqrt(p (1 - p) / (N H)): derived
    from the binomial, not tuned (u is uniform on multiples of 2^-24, so P(u >= p) differs from 1 - p by less than 2^-24)."""
    N, H = 4096, 128
    frac = float(_dev_mask(N, H, p, SEED, 0, 0, None, _dev()).mean())
    sigma = np.sqrt(p * (1 - p) / (N * H))
    print(f"p={p}: kept {frac:.6f}, expected {1 - p}, {abs(frac - (1 - p)) / sigma:.2f} sigma")
    assert abs(frac - (1 - p)) <= 5 * sigma


# ---- 4. the model in training mode --------------------------------------------------------------------------------------------
# (fixture whose graph and inputs are used, H, L, batch_norm)
# (h128_ln: the chained LayerNorm backward exists at H = 128 only)
CONFIGS = {"h128_bn": ("tiny_h128l8_s0.npz", 128, 2, True), "h32_ln": ("tiny_h32l2ln_s0.npz", 32, 2, False),
           "h128_ln": ("tiny_h128l8_s0.npz", 128, 2, False)}
# every backward schedule a pass with p > 0 can reach (engine.Options switches set away from their defaults); NODE_FUSED is pinned
# off by the forward whatever is asked for
SCHEDULES = {
    "default": {}, "node_fused_off": {"NODE_FUSED": False}, "chain_no_plan": {"TWO_SIDED": False}, "layerwise_sweep": {"CHAIN": False},
    "layerwise": {"CHAIN": False, "TWO_SIDED": False}, "unfused": {"FUSED": False}, "one_stream": {"TN_SIDE": False},
    "tn_now": {"TN_AT": "now"}, "tn_no_split": {"TN_SPLIT": False}, "fwd_separate": {"TWO_SIDED_FWD": False},
    "ln_no_sweep": {"LN_SWEEP": False},
}
P = 0.5
_CASES = {}


def _case(name):
    if name in _CASES:
        return _CASES[name]
    from gnnome_assembly_amd import synth
    fname, H, L, bn = CONFIGS[name]
    z = np.load(os.path.join(GOLDEN, fname))
    c = dict(src=z["src"], dst=z["dst"], n=int(z["n"]), e=z["e_raw"], pe=z["pe"], y=z["y"], pw=float(z["pos_weight"]),
             sd=synth.synth_state_dict(H, L, seed=3), H=H, L=L, bn=bn)
    _CASES[name] = c
    return c


def _step(c, switches=None, dropout=P, seed=SEED, step=0, checkpoint=0, mode="train", keyword=True):
    """One step of a fresh model on cuda:0 with the device's dropout stream set to (seed, step)."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import engine
    dev = _dev()
    kw = dict(dropout=dropout) if keyword else {}
    model = G.GraphGatedGCNModel(1, 2, c["H"], 16, c["L"], 64, c["bn"], 16, **kw)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in c["sd"].items()})
    model.to(dev)
    model.activation_checkpoint = checkpoint
    g = G.AssemblyGraph(c["src"], c["dst"], c["n"]).to(dev)
    e, pe, y = (torch.from_numpy(c[k]).to(dev) for k in ("e", "pe", "y"))
    engine.dropout_seed(seed, step, dev)
    with engine.options(**(switches or {})):
        if mode == "train":
            s = model(g, None, e, pe)
            loss = G.BCEWithLogitsLoss(c["pw"])(s.squeeze(-1), y)
            loss.backward()
        else:
            if mode == "eval":
                model.eval()
            with torch.no_grad() if mode == "no_grad" else torch.enable_grad():
                s = model(g, None, e, pe)
            loss = None
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()} if mode == "train" else None
    return dict(s=s.detach().cpu(), loss=None if loss is None else loss.item(), grads=grads, drop=model.last_dropout)


def _oracle(c, drop):
    """fp64 torch restatement: the oracle's layer function with the exported masks (caller's node numbering) times
    float32(1 / (1 - p)) multiplied in behind every layer.  Cached per (configuration, p, key, step)."""
    key = ("oracle",) + tuple(drop)
    if key in c:
        return c[key]
    from gnnome_assembly_amd import engine
    dev = _dev()
    sd = sd_to_torch(c["sd"], torch.float64, requires_grad=True)
    src, dst = torch.from_numpy(c["src"]).long(), torch.from_numpy(c["dst"]).long()
    h = torch.from_numpy(c["pe"]).double() @ sd["linear_pe.weight"].t() + sd["linear_pe.bias"]
    e = torch.relu(torch.from_numpy(c["e"]).double() @ sd["linear1_edge.weight"].t() + sd["linear1_edge.bias"])
    e = e @ sd["linear2_edge.weight"].t() + sd["linear2_edge.bias"]
    masks = []
    for i in range(c["L"]):
        h, e = orc.layer_forward(sd, i, src, dst, c["n"], h, e, c["bn"])
        m = engine.dropout_mask(c["n"], c["H"], drop, i, dev).cpu()
        masks.append(m.numpy().astype(bool))
        h = h * (m.double() * float(ref.scale_of(drop[0])))
    s = orc.predictor_forward(sd, src, dst, h, e)
    loss = orc.bce_loss(s, torch.from_numpy(c["y"]).double(), c["pw"])
    loss.backward()
    c[key] = dict(s=s.detach().numpy(), loss=loss.item(), grads={k: v.grad.numpy() for k, v in sd.items()}, masks=masks)
    return c[key]


def _vs_oracle(res, o, what):
    assert_parity(res["s"].numpy(), o["s"], f"{what} logits")
    assert abs(res["loss"] - o["loss"]) < 1e-5, (what, res["loss"], o["loss"])
    floor = max(GRAD_ABS_FLOOR, 1e-6 * max(float(np.linalg.norm(v)) for v in o["grads"].values()))
    bad = []
    for k, want in o["grads"].items():
        got = res["grads"][k].double().numpy()
        r, mx = rel_l2(got, want), float(np.abs(got - want).max())
        if not (r <= GRAD_L2 or mx <= floor):
            bad.append((k, r, mx))
    assert not bad, (what, bad)


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_model_training_step_vs_fp64(cfg, sched):
    c = _case(cfg)
    res = _step(c, SCHEDULES[sched])
    assert res["drop"] == (P, SEED, 0)
    o = _oracle(c, res["drop"])
    for i, m in enumerate(o["masks"]):          # the exported masks are the restatement's, and they are not trivial
        assert np.array_equal(m, ref.keep_mask(np.arange(c["n"]), c["H"], P, SEED, 0, i)) and 0.3 < m.mean() < 0.7
    _vs_oracle(res, o, f"{cfg} {sched}")


def test_node_fused_cannot_be_forced_onto_a_dropout_backward():
    """NODE_FUSED takes the BatchNorm_h backward sums of the unmasked gradient inside the projection backward: the forward saves
    its options with the switch pinned off, and a backward that is handed the switch explicitly is refused, never run unmasked."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import _lib, engine
    dev = _dev()
    c = _case("h128_bn")
    g = G.AssemblyGraph(c["src"], c["dst"], c["n"]).to(dev)
    Pm = {k: v.to(dev) for k, v in sd_to_torch(c["sd"]).items()}
    e, pe = torch.from_numpy(c["e"]).to(dev), torch.from_numpy(c["pe"]).to(dev)
    with engine.options(NODE_FUSED=True):
        s, ms = engine.model_forward(g, e, pe, Pm, c["L"], True, True, dropout=(P, SEED, 0))
        s0, ms0 = engine.model_forward(g, e, pe, Pm, c["L"], True, True)
    assert ms.opts.NODE_FUSED is False and ms0.opts.NODE_FUSED is True and ms.dropout == (P, SEED, 0) and ms0.dropout is None
    with pytest.raises(_lib.GnmError, match="NODE_FUSED"):
        engine.model_backward(g, Pm, c["L"], ms, torch.ones_like(s), True, opts=engine.current().replace(NODE_FUSED=True))


# ---- 5. recompute -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["checkpoint1", "checkpoint2", "lean"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_recompute_is_bit_identical(cfg, how):
    """activation_checkpoint = 1 / 2 and the lean activation mode re-derive the masks from the saved (p, key, step): logits and
    gradients are the saved mode's bits.  Segments of one layer run under CHAIN=False in both modes: the chained schedule of a
    segment is that of a model of the segment's depth, another order of the same sums (tests/test_gpu_checkpoint.py), and this
    test is about the masks."""
    c = _case(cfg)
    sw = {"ACTIVATIONS": "saved", "CHAIN": how != "checkpoint1"}
    key = ("saved", sw["CHAIN"])
    if key not in c:
        c[key] = _step(c, sw)
    base = c[key]
    res = _step(c, dict(sw, ACTIVATIONS="lean")) if how == "lean" else _step(c, sw, checkpoint=int(how[-1]))
    assert torch.equal(res["s"], base["s"]) and res["loss"] == base["loss"], how
    for k, v in base["grads"].items():
        assert torch.equal(res["grads"][k], v), (how, k)
    assert not torch.equal(base["s"], _step(c, dropout=0.0)["s"])           # (and the masks did something)


# ---- 6. seed and step ---------------------------------------------------------------------------------------------------------
def test_seed_and_step():
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import engine
    dev = _dev()
    c = _case("h128_bn")
    model = G.GraphGatedGCNModel(1, 2, c["H"], 16, c["L"], 64, c["bn"], 16, dropout=P)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in c["sd"].items()})
    model.to(dev)
    g = G.AssemblyGraph(c["src"], c["dst"], c["n"]).to(dev)
    e, pe = torch.from_numpy(c["e"]).to(dev), torch.from_numpy(c["pe"]).to(dev)

    def two():
        out = []
        for _ in range(2):
            s = model(g, None, e, pe).detach().cpu()
            out.append((s, model.last_dropout, engine.dropout_mask(c["n"], c["H"], model.last_dropout, 0, dev).cpu()))
        return out
    engine.dropout_seed(SEED, device=dev)
    a = two()
    assert a[0][1] == (P, SEED, 0) and a[1][1] == (P, SEED, 1)              # one step per training forward
    assert not torch.equal(a[0][2], a[1][2]) and not torch.equal(a[0][0], a[1][0])
    engine.dropout_seed(SEED, device=dev)
    b = two()
    for x, y in zip(a, b):
        assert x[1] == y[1] and torch.equal(x[2], y[2]) and torch.equal(x[0], y[0])
    engine.dropout_seed(SEED + 1, device=dev)
    assert not torch.equal(two()[0][2], a[0][2])
    model.eval()                                                             # no draw, no step outside training
    before = model.last_dropout
    model(g, None, e, pe)
    with torch.no_grad():
        model.train()(g, None, e, pe)
    assert model.last_dropout == before and engine.dropout_draw(P, dev)[2] == before[2] + 1
    # two ranks' keys differ, and with them the masks
    k0, k1 = engine.dropout_key(SEED, 0), engine.dropout_key(SEED, 1)
    assert k0 == SEED and k1 == SEED ^ 0x9E3779B97F4A7C15
    m0, m1 = (engine.dropout_mask(c["n"], c["H"], (P, k, 0), 0, dev).cpu() for k in (k0, k1))
    assert 0.4 < float((m0 != m1).float().mean()) < 0.6


# ---- 7. off is off ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_off_is_off(cfg):
    """dropout=0.0 is the model built without the keyword, bit for bit and launch for launch; eval() and no_grad() at p = 0.5
    give those logits too."""
    from gnnome_assembly_amd import engine
    c = _case(cfg)
    plain = _step(c, keyword=False)
    zero = _step(c, dropout=0.0)
    assert zero["drop"] is None and torch.equal(zero["s"], plain["s"]) and zero["loss"] == plain["loss"]
    for k, v in plain["grads"].items():
        assert torch.equal(zero["grads"][k], v), k
    for mode in ("eval", "no_grad"):
        r = _step(c, mode=mode)
        assert r["drop"] is None and torch.equal(r["s"], plain["s"]), mode
    ops = {}
    for p in (0.0, P):          # NODE_FUSED off for both: p > 0 pins it off, and this compares launch lists
        engine.profile_ops(True)
        try:
            _step(c, {"NODE_FUSED": False}, dropout=p)
        finally:
            ops[p] = engine.profile_ops(False)
    assert "gnm_node_dropout_apply" not in ops[0.0]
    assert ops[P]["gnm_node_dropout_apply"][0] == 2 * c["L"]               # per layer: once forward, once on the gradient
    assert {k: n for k, (n, _) in ops[0.0].items()} == {k: n for k, (n, _) in ops[P].items() if k != "gnm_node_dropout_apply"}


# ---- the stack alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,bn", [(128, True), (32, False), (48, True)])
def test_stack_alone_takes_the_engine_route(H, bn):
    """layers.GraphGatedGCN(dropout=0.5) on a graph with an internal node order of its own: outputs and the input gradients
    against the fp64 restatement with the exported masks (caller's numbering: the internal order must not show).  48: a width
    run zero-padded to 128, whose masks are those of the real width."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import engine, synth
    dev = _dev()
    L = 2
    src, dst, n = synth.make_graph(60, seed=9, permute_edge_ids=True)
    rng = np.random.default_rng(H)
    nrank = torch.from_numpy(rng.permutation(n)).to(dev)
    g = G.AssemblyGraph.from_tensors(torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev), n, nrank)
    assert "nperm" in g.index(dev)
    sd = {k[4:]: v for k, v in synth.synth_state_dict(H, L, seed=5).items() if k.startswith("gnn.")}
    stack = G.layers.GraphGatedGCN(L, H, bn, dropout=P)
    stack.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    stack.to(dev)
    h0, e0 = rng.standard_normal((n, H)).astype(np.float32), rng.standard_normal((src.size, H)).astype(np.float32)
    wh, we = rng.standard_normal((n, H)), rng.standard_normal((src.size, H))
    h = torch.from_numpy(h0).to(dev).requires_grad_(True)
    e = torch.from_numpy(e0).to(dev).requires_grad_(True)
    engine.dropout_seed(SEED, 5, dev)
    ho, eo = stack(g, h, e)
    assert stack.last_dropout == (P, SEED, 5)
    ((ho * torch.from_numpy(wh).float().to(dev)).sum() + (eo * torch.from_numpy(we).float().to(dev)).sum()).backward()
    torch.cuda.synchronize()
    p64 = {"gnn." + k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd.items()}
    h64, e64 = torch.from_numpy(h0).double().requires_grad_(True), torch.from_numpy(e0).double().requires_grad_(True)
    hh, ee = h64, e64
    for i in range(L):
        hh, ee = orc.layer_forward(p64, i, torch.from_numpy(src).long(), torch.from_numpy(dst).long(), n, hh, ee, bn)
        m = engine.dropout_mask(n, H, stack.last_dropout, i, dev).cpu()
        assert np.array_equal(m.numpy().astype(bool), ref.keep_mask(np.arange(n), H, P, SEED, 5, i))
        hh = hh * (m.double() * float(ref.scale_of(P)))
    ((hh * torch.from_numpy(wh)).sum() + (ee * torch.from_numpy(we)).sum()).backward()
    assert torch.equal(ho.detach().cpu() == 0, (m == 0) | (hh.detach() == 0))       # dropped exactly where the last mask says
    assert_parity(ho.detach().cpu().numpy(), hh.detach().numpy(), "stack h")
    assert_parity(eo.detach().cpu().numpy(), ee.detach().numpy(), "stack e")
    gmax = max(float(v.grad.norm()) for v in p64.values())
    for name, got, want in [("d h", h.grad, h64.grad), ("d e", e.grad, e64.grad)] + [
            (k, dict(stack.named_parameters())[k[4:]].grad, v.grad) for k, v in p64.items()]:
        got, want = got.detach().cpu().double().numpy(), want.numpy()
        r, mx = rel_l2(got, want), float(np.abs(got - want).max())
        assert r <= GRAD_L2 or mx <= max(GRAD_ABS_FLOOR, 1e-6 * gmax), (name, r, mx)
    stack.eval()
    h1, _ = stack(g, h.detach(), e.detach())
    stack.dropout = 0.0
    h2, _ = stack.train()(g, h.detach(), e.detach())
    assert torch.equal(h1, h2)                                               # eval mode: the per-layer route, no mask
