"""CPU suite for the device loss / metrics of the onset training step (syncfusion_amd/onset_loss.py, sf_op_onset_*): the ``loss=`` choice of
``OnsetModel``, the untouched default, the C-ABI symbols, the refusals of ``GraphedOnsetTrainStep`` that need no device, and the fp64
restatement of the metrics (tests/onset_metrics_ref.py) against ``BCLoss.evaluate``.  No kernel runs here."""
import math
import os
import re

import numpy as np
import pytest
import torch

import onset_metrics_ref as ref
from helpers import ROOT

LOSS_SYMBOLS = ("sf_op_onset_loss_workspace_bytes", "sf_op_onset_bce_fwd", "sf_op_onset_bce_bwd", "sf_op_onset_metrics")


def _model(**kw):
    from syncfusion_amd import OnsetModel, VideoOnsetNet

    return OnsetModel(1e-4, 0.9, 0.999, 1e-8, 1e-2, VideoOnsetNet(False), **kw)


def test_loss_choice_is_validated():
    from syncfusion_amd.module_onset import BCLoss
    from syncfusion_amd.onset_loss import DeviceBCLoss

    m = _model(loss="hip")
    assert isinstance(m.loss, DeviceBCLoss) and m.loss.threshold == 0.75
    assert callable(m.loss.evaluate) and not list(m.loss.parameters())
    assert list(m.state_dict().keys()) == list(_model().state_dict().keys())      # the loss adds nothing to a checkpoint
    assert isinstance(_model(loss="torch").loss, BCLoss)
    for bad in ("HIP", "device", "", None):
        with pytest.raises(ValueError, match="loss must be one of"):
            _model(loss=bad)


def test_default_is_bcloss_with_python_floats():
    from syncfusion_amd.module_onset import BCLoss

    m = _model()
    assert type(m.loss) is BCLoss
    g = torch.Generator().manual_seed(0)
    out = m.loss.evaluate(torch.randn(3, 10, generator=g), (torch.rand(3, 10, generator=g) < 0.4).float())
    assert set(out) == {"AP", "Acc", "OnsNumAcc"}
    assert all(isinstance(v, float) for v in out.values())      # (numpy's float64 is a Python float)


def test_loss_symbols_declared_bound_and_exported():
    import syncfusion_amd
    from syncfusion_amd import _lib

    header = open(os.path.join(ROOT, "include", "syncfusion_amd.h")).read()
    declared = set(re.findall(r"\b(sf_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in LOSS_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/syncfusion_amd.h"
        assert name in _lib.SYMBOLS, f"{name} is not bound in _lib.py"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert "GraphedOnsetTrainStep" in syncfusion_amd.__all__ and syncfusion_amd.GraphedOnsetTrainStep is syncfusion_amd.onset_training.GraphedOnsetTrainStep
    # the workspace query is host-only: one bound for loss and metrics, growing with n
    ws = lib.sf_op_onset_loss_workspace_bytes
    assert ws(0) == -1 and ws(-3) == -1 and ws(1 << 31) == -1
    assert ws(1) >= 64 + 8 + 4 and ws(480) >= 64 + 8 * 241 + 4 * 480
    assert ws(1 << 20) >= max(3 * 8 * 256, 64 + 8 * ((1 << 19) + 1) + 4 * (1 << 20))
    assert all(ws(n) % 8 == 0 and ws(n + 1) >= ws(n) for n in (1, 2, 63, 64, 255, 4096, 4097, 65535))


def test_calls_check_their_arguments():
    """Null pointers, bad sizes, a short or misaligned workspace are refused before anything is launched (no device is touched)."""
    from syncfusion_amd import _lib

    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.float64)
    p = buf.data_ptr()
    assert lib.sf_op_onset_bce_fwd(None, p, 4, p, p, p, 1 << 20, None) != 0 and b"null" in lib.sf_last_error()
    assert lib.sf_op_onset_bce_fwd(p, p, 0, p, p, p, 1 << 20, None) != 0
    assert lib.sf_op_onset_bce_fwd(p, p, 4, p, p, p, 8, None) != 0 and b"workspace" in lib.sf_last_error()
    assert lib.sf_op_onset_bce_fwd(p, p, 4, p, p, p + 4, 1 << 20, None) != 0 and b"misaligned" in lib.sf_last_error()
    assert lib.sf_op_onset_bce_bwd(p, p, p, None, 4, p, None) != 0 and b"null" in lib.sf_last_error()
    assert lib.sf_op_onset_bce_bwd(p, p, p, p, 0, p, None) != 0
    assert lib.sf_op_onset_metrics(p, p, 0, 4, 0.75, p, p, 1 << 20, None) != 0
    assert lib.sf_op_onset_metrics(p, p, 4, 4, 0.75, None, p, 1 << 20, None) != 0 and b"null" in lib.sf_last_error()
    assert lib.sf_op_onset_metrics(p, p, 4, 4, 0.75, p, p, 16, None) != 0 and b"workspace" in lib.sf_last_error()
    assert lib.sf_op_onset_metrics(p, p, 1 << 13, 1 << 12, 0.75, p, p, 1 << 40, None) != 0 and b"2^24" in lib.sf_last_error()


def test_device_loss_has_no_cpu_path():
    from syncfusion_amd._lib import SyncFusionAmdError
    from syncfusion_amd.onset_loss import balanced_bce, step_metrics

    with pytest.raises(SyncFusionAmdError):
        balanced_bce(torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(SyncFusionAmdError):
        step_metrics(torch.zeros(2, 3), torch.zeros(2, 3))


def test_graphed_step_refusals_need_no_device():
    from syncfusion_amd import GraphedOnsetTrainStep

    batch = {"frames": torch.zeros(1, 3, 2, 16, 16), "label": torch.zeros(1, 2)}
    with pytest.raises(ValueError, match='loss="hip"'):
        GraphedOnsetTrainStep(_model(), batch)
    m = _model(loss="hip")
    with pytest.raises(TypeError, match="syncfusion_amd.optim.AdamW"):
        GraphedOnsetTrainStep(m, batch, optimizer=torch.optim.AdamW(m.parameters()))


@pytest.mark.parametrize("seed", range(6))
def test_reference_helper_matches_bcloss_evaluate(seed):
    from syncfusion_amd.module_onset import BCLoss

    rng = np.random.default_rng(seed)
    for _ in range(12):
        N, T = int(rng.integers(1, 9)), int(rng.integers(2, 40))
        z = ref.grid_logits(rng, (N, T))
        if rng.random() < 0.5:                                   # heavy ties
            z = rng.choice(np.array([-1.0, 0.5, 2.0, 20.0, 25.0, 30.0], dtype=np.float32), size=(N, T))
        t = ref.random_labels(rng, (N, T), float(rng.choice([0.05, 0.3, 0.5, 0.9])))
        t.reshape(-1)[0], t.reshape(-1)[-1] = 1.0, 0.0            # two classes: BCLoss.evaluate raises on one
        want = BCLoss().evaluate(torch.from_numpy(z), torch.from_numpy(t))
        got = ref.step_metrics_ref(z, t)
        assert got["b"] >= 1
        assert abs(got["AP"] - want["AP"]) <= 1e-12, (N, T, got, want)
        assert got["Acc"] == want["Acc"] and got["OnsNumAcc"] == want["OnsNumAcc"], (N, T, got, want)


def test_reference_helper_edge_cases():
    # one class: empty subset -> NaN, OnsNumAcc still defined
    z = np.array([[2.0, 2.0, -2.0]], dtype=np.float32)
    m = ref.step_metrics_ref(z, np.zeros((1, 3), dtype=np.float32))
    assert math.isnan(m["AP"]) and math.isnan(m["Acc"]) and m["OnsNumAcc"] == 0.0 and m["b"] == 0
    # runs of 1..5 keep ceil(L / 2); runs do not join across rows
    for L in range(1, 6):
        z = np.full((2, 6), -2.0, dtype=np.float32)
        z[0, 6 - L:] = 2.0
        z[1, :L] = 2.0
        t = np.zeros((2, 6), dtype=np.float32)
        t[0, :(L + 1) // 2] = 1.0
        t[1, :(L + 1) // 2] = 1.0
        assert ref.step_metrics_ref(z, t)["OnsNumAcc"] == 1.0, L
    # equal logits are equal scores wherever they sit
    z = np.tile(np.array([0.3, 1.7, -0.9], dtype=np.float32), 50).reshape(1, -1)
    assert len(np.unique(ref.sigmoid32(z))) == 3
