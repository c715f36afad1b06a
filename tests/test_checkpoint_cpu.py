"""Layer-segment activation checkpointing, the part that needs no device: the segment arithmetic the forward, the backward and
the GPU tests share (engine.checkpoint_segments), the model attribute and its environment default, the argument check, and
that checkpointing did NOT become a schedule switch (engine.Options is what tests/helpers.py's schedule matrix spans).
test_checkpointing_is_not_a_schedule_switch is a guard -- it holds with or without the feature; the others need it."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPTION_NAMES = ("FUSED", "ACTIVATIONS", "CHAIN", "TN_SIDE", "TN_SIDE_CAP", "SRC_SIDE_CAP", "TN_AT", "TN_SPLIT", "TWO_SIDED",
                "TWO_SIDED_FWD", "WIDE_FUSED", "NODE_FUSED", "LN_SWEEP")


def test_checkpoint_segments():
    from gnnome_assembly_amd import engine
    assert engine.checkpoint_segments(8, 3) == [(0, 3), (3, 6), (6, 8)]
    assert engine.checkpoint_segments(16, 4) == [(0, 4), (4, 8), (8, 12), (12, 16)]
    assert engine.checkpoint_segments(2, 5) == [(0, 2)]
    assert engine.checkpoint_segments(8, 0) == []
    assert engine.checkpoint_segments(8, 1) == [(i, i + 1) for i in range(8)]
    assert engine.checkpoint_segments(8, 8) == [(0, 8)]
    for L in range(1, 20):          # a partition of the stack, in order, no segment longer than k
        for k in range(1, 22):
            segs = engine.checkpoint_segments(L, k)
            assert [i for a, b in segs for i in range(a, b)] == list(range(L))
            assert all(0 < b - a <= k for a, b in segs) and len(segs) == -(-L // k)


def _new_model():
    import gnnome_assembly_amd as G
    return G.GraphGatedGCNModel(1, 2, 32, 16, 2, 64, True, 16)


def test_a_fresh_model_does_not_checkpoint(monkeypatch):
    monkeypatch.delenv("GNM_CHECKPOINT", raising=False)
    m = _new_model()
    assert m.activation_checkpoint == 0 and type(m.activation_checkpoint) is int
    m.activation_checkpoint = 3           # a plain attribute: no parameter, no buffer, not in the state_dict
    assert m.activation_checkpoint == 3
    assert not any("checkpoint" in k for k in m.state_dict())


def test_environment_sets_the_default_of_new_models():
    code = ("import gnnome_assembly_amd as G\n"
            "print('ckpt', G.GraphGatedGCNModel(1, 2, 32, 16, 2, 64, True, 16).activation_checkpoint)\n")
    env = dict(os.environ, GNM_CHECKPOINT="4", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "ckpt 4" in out.stdout.splitlines()


def test_checkpointing_is_not_a_schedule_switch():
    from gnnome_assembly_amd import engine
    assert engine._OPTION_NAMES == OPTION_NAMES
    assert not hasattr(engine.current(), "CHECKPOINT")
    with pytest.raises(engine._lib.GnmError):
        engine.current().replace(CHECKPOINT=2)


@pytest.mark.parametrize("bad", [-1, 1.5, "4", None])
def test_a_bad_value_is_refused(bad):
    """model_forward's argument check (the first thing it does), called directly: no device needed."""
    from gnnome_assembly_amd import engine
    with pytest.raises(engine._lib.GnmError):
        engine._checkpoint_arg(bad)
    with pytest.raises(engine._lib.GnmError):
        engine.checkpoint_segments(8, bad)


def test_good_values_pass_the_check():
    import numpy as np
    from gnnome_assembly_amd import engine
    assert [engine._checkpoint_arg(k) for k in (0, 1, 16, np.int64(3))] == [0, 1, 16, 3]
