"""CPU suite for the onset net's training surface: BCLoss and its metrics (main/module_onset.py:268-354), the OnsetModel drop-in's
optimizer and checkpoint keys, and the training ops' C-ABI symbols (no compute calls)."""
import math

import numpy as np
import pytest
import torch


def test_bcloss_forward_matches_weighted_bce():
    from syncfusion_amd.module_onset import BCLoss

    g = torch.Generator().manual_seed(0)
    pred = torch.randn(3, 10, generator=g)                     # fp32 logits (the reference casts the target to float)
    target = (torch.rand(3, 10, generator=g) < 0.3).long()
    n, pos = target.numel(), target.sum()
    ref = torch.nn.BCEWithLogitsLoss(pos_weight=(n - pos) / pos)(pred.view(-1), target.view(-1).float())
    assert torch.equal(BCLoss()(pred, target), ref)
    # by hand, fp64: mean over frames of -(w t log s(p) + (1 - t) log(1 - s(p))),  w = (n - sum t) / sum t
    s = torch.sigmoid(pred.double().view(-1))
    t = target.double().view(-1)
    hand = -((n - pos) / pos * t * torch.log(s) + (1 - t) * torch.log(1 - s)).mean()
    assert float(BCLoss()(pred, target)) == pytest.approx(float(hand), rel=1e-6)


def test_bcloss_without_positives_is_not_finite():
    from syncfusion_amd.module_onset import BCLoss

    loss = BCLoss()(torch.zeros(2, 4), torch.zeros(2, 4))   # pos_weight = inf, as in the reference
    assert not math.isfinite(float(loss))


def _logit(p):
    return torch.log(torch.tensor(p, dtype=torch.float64) / (1 - torch.tensor(p, dtype=torch.float64)))


def test_evaluate_hand_computed():
    from syncfusion_amd.module_onset import BCLoss

    # probabilities after the sigmoid; targets (2 clips x 5 frames)
    p = [[0.9, 0.8, 0.1, 0.2, 0.95],
         [0.3, 0.6, 0.85, 0.9, 0.1]]
    t = [[1, 0, 0, 0, 1],
         [0, 1, 1, 0, 0]]
    pred, target = _logit(p), torch.tensor(t, dtype=torch.float64)
    m = BCLoss().evaluate(pred, target)
    # balance: 4 positives (flat idx 0, 4, 6, 7), the first 4 negatives (1, 2, 3, 5)
    # scores: pos 0.9, 0.95, 0.6, 0.85; neg 0.8, 0.1, 0.2, 0.3
    # ranking 0.95+ 0.9+ 0.85+ 0.8- 0.6+ 0.3- 0.2- 0.1-: AP = (1 + 1 + 1 + 4/5) / 4 = 0.95
    assert m["AP"] == pytest.approx(0.95, abs=1e-12)
    # > 0.75: 0.95 0.9 0.85 0.8 -> 1 (pos, pos, pos, neg); 0.6 -> 0 (pos): correct 3 + 3 of 8
    assert m["Acc"] == pytest.approx(6 / 8, abs=1e-12)
    # onset counts: clip 0 pred 1 1 0 0 1 -> consecutive removal 1 0 0 0 1 = 2 (target 2: hit);
    # clip 1 pred 0 0 1 1 0 -> 0 0 1 0 0 = 1 (target 2: miss)
    assert m["OnsNumAcc"] == pytest.approx(0.5, abs=1e-12)


def test_average_precision_against_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    from syncfusion_amd.module_onset import average_precision

    rng = np.random.default_rng(1)
    for _ in range(20):
        t = rng.integers(0, 2, 64)
        t[0] = 1
        s = np.round(rng.random(64), 2)     # ties included
        assert average_precision(t, s) == pytest.approx(sk.average_precision_score(t, s), abs=1e-12)


def test_configure_optimizers_hyperparameters():
    from syncfusion_amd import OnsetModel, VideoOnsetNet

    m = OnsetModel(2e-4, 0.85, 0.99, 1e-7, 0.05, VideoOnsetNet(False))
    opt = m.configure_optimizers()
    assert isinstance(opt, torch.optim.AdamW)
    (group,) = opt.param_groups
    assert group["lr"] == 2e-4 and group["betas"] == (0.85, 0.99) and group["eps"] == 1e-7 and group["weight_decay"] == 0.05
    assert len(group["params"]) == len(list(m.model.parameters()))


def test_state_dict_keys_match_reference_layout():
    from syncfusion_amd import OnsetModel, VideoOnsetNet

    m = OnsetModel(1e-4, 0.9, 0.999, 1e-8, 1e-2, VideoOnsetNet(False))
    keys = list(m.state_dict().keys())
    assert len(keys) == 226
    assert keys[0] == "model.net.model.stem.0.weight" and keys[-1] == "model.fc.2.bias"
    assert all(k.startswith(("model.net.model.", "model.fc.")) for k in keys)
    assert "model.net.model.layer4.1.conv2.1.num_batches_tracked" in keys


def test_training_op_symbols_exported():
    from syncfusion_amd import _lib

    lib = _lib.load()
    names = ["sf_op_vconv_workspace_bytes", "sf_op_vconv_fwd", "sf_op_vconv_bwd", "sf_op_bn_train_workspace_bytes", "sf_op_bn_train_fwd",
             "sf_op_bn_train_bwd", "sf_op_video_to_cl", "sf_op_video_pool", "sf_op_video_pool_bwd"]
    for n in names:
        assert hasattr(lib, n), n
        assert n in _lib.SYMBOLS, n
    # workspace queries are host-only: a shape error comes back as -1, a valid one as a positive byte count
    d = _lib.VConvDesc(2, 4, 16, 16, 64, 64, 144, 192, 1, 3, 3, 2, 2, 0, 1, 1)
    assert lib.sf_op_vconv_workspace_bytes(d) > 0
    bad = _lib.VConvDesc(2, 4, 16, 16, 64, 60, 144, 192, 1, 3, 3, 2, 2, 0, 1, 1)   # cin_ld not a multiple of 4
    assert lib.sf_op_vconv_workspace_bytes(bad) == -1
    assert lib.sf_op_bn_train_workspace_bytes(1000, 45) > 0 and lib.sf_op_bn_train_workspace_bytes(1, 45) == -1
