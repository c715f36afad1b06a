"""CPU: the opt-in for LayerNorm layers wider than 256 channels (layers.WIDE_LAYERNORM / GNM_WIDE_LN) -- module surface with the
switch on and off, and the C ABI of the kernels behind it (gnm_ln_wide_*: declared in include/gnm.h, bound in _lib.SIGNATURES,
exported by the library)."""
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_ENTRY_POINTS = ("gnm_ln_wide_row_stats", "gnm_ln_wide_edge_gate_fwd", "gnm_ln_wide_node_update_fwd", "gnm_ln_wide_node_bwd_sums",
                     "gnm_ln_wide_node_bwd_apply", "gnm_ln_wide_edge_bwd_sums", "gnm_ln_wide_edge_bwd_apply")


def _layer_schema(cin, cout):
    keys = [f"{k}.{w}" for k in ("A_1", "A_2", "A_3", "B_1", "B_2", "B_3") for w in ("weight", "bias")]
    shapes = {k: ((cout, cin) if k.endswith("weight") else (cout,)) for k in keys}
    for k in ("bn_h.weight", "bn_h.bias", "bn_e.weight", "bn_e.bias"):      # nn.LayerNorm(out_channels): weight, bias, no buffers
        shapes[k] = (cout,)
    return shapes


def test_switch_on_wide_layernorm_modules_construct_with_the_reference_schema(monkeypatch):
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import layers, synth
    monkeypatch.setattr(layers, "WIDE_LAYERNORM", True)
    conv = G.layers.GatedGCN_1d(32, 300, False)
    assert conv._wide_ln is True and not conv.residual and not conv.batch_norm
    sd = conv.state_dict()
    want = _layer_schema(32, 300)
    assert list(sd) == list(want) and all(tuple(sd[k].shape) == want[k] for k in want)
    m = G.GraphGatedGCNModel(1, 2, 512, 16, 1, 64, False, 16)
    assert m._wide_ln() is True
    ref = synth.synth_state_dict(512, 1, 0)
    sd = m.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    assert all(tuple(sd[k].shape) == ref[k].shape for k in ref)
    assert not any("running" in k or "num_batches" in k for k in sd)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in ref.items()}, strict=True)
    assert layers.padded_width(300) == 512 and layers.padded_width(600) == 768
    # the decision is the layer's, taken at construction: flipping the switch afterwards changes nothing about it
    monkeypatch.setattr(layers, "WIDE_LAYERNORM", False)
    assert conv._wide_ln is True and m._wide_ln() is True


def test_switch_off_is_the_default_and_keeps_refusing(monkeypatch):
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import layers
    if os.environ.get("GNM_WIDE_LN", "0") != "1":
        assert layers.WIDE_LAYERNORM is False
    monkeypatch.setattr(layers, "WIDE_LAYERNORM", False)
    with pytest.raises(NotImplementedError, match="LayerNorm"):
        G.layers.GatedGCN_1d(32, 300, False)
    with pytest.raises(NotImplementedError, match="LayerNorm"):
        G.GraphGatedGCNModel(1, 2, 512, 16, 1, 64, False, 16)
    G.layers.GatedGCN_1d(32, 300, True), G.layers.GatedGCN_1d(48, 256, False)        # what was legal stays legal


def test_wide_layernorm_entry_points_are_declared_bound_and_exported():
    from gnnome_assembly_amd import _lib
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gnm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gnm_ln_wide_\w+)\s*\(", hdr))
    assert declared == set(WIDE_ENTRY_POINTS)
    for name in WIDE_ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name
    assert lib.gnm_abi_version() == 7       # additive: the ABI stays where it was
