"""GPU suite for the device end of the onset training step (syncfusion_amd/onset_loss.py over csrc/onset_loss.hip): the class-balanced BCE
loss and its gradient against fp64 autograd of ``BCLoss``, the step metrics against the fp64 restatement of tests/onset_metrics_ref.py and
against ``BCLoss.evaluate`` itself, the absence of host synchronisation, and the whole training step with ``loss="hip"`` against the fp64
oracle step of tests/test_gpu_onset_train.py.

Every logit lies on a 1/64 grid with |z| <= 8, none within 1e-2 of ln 3 (``onset_metrics_ref.grid_logits``), plus -- where stated -- the
saturated group {20, 25, 30}, each of which is exactly 1.0f under any fp32 sigmoid: ordering, ties and threshold decisions of the fp32
scores are unambiguous, so the helper alone determines every expected value."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

import onset_metrics_ref as ref
from test_gpu_onset_train import NET_TOL, TOL, _labels, _oracle_step, _seeded_net, _worst
from helpers import rel_l2

pytestmark = pytest.mark.gpu

LOSS_SHAPES = [(1, 2), (2, 3), (7, 37), (16, 30), (64, 30), (33, 257), (257, 255), (1024, 1024)]   # the last: 2^20 logits, 256 workgroups
UPSTREAM = 3.25


@functools.lru_cache(maxsize=None)
def _loss_case(shape):
    """Inputs and the fp64 reference (BCLoss + autograd on the CPU) of one shape, computed once."""
    from syncfusion_amd.module_onset import BCLoss

    rng = np.random.default_rng(1000 + shape[0] * 7 + shape[1])
    z = ref.grid_logits(rng, shape)
    t = ref.random_labels(rng, shape, 0.3)
    t.reshape(-1)[0], t.reshape(-1)[-1] = 1.0, 0.0     # both classes: without a positive the loss is NaN, without a negative it is exactly 0
    zd = torch.from_numpy(z).double().requires_grad_()
    loss = BCLoss()(zd, torch.from_numpy(t).double())
    loss.backward()
    return torch.from_numpy(z), torch.from_numpy(t), loss.detach(), zd.grad.detach()


@pytest.mark.autograd
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=[f"{a}x{b}" for a, b in LOSS_SHAPES])
def test_loss_and_gradient_vs_fp64(cuda, shape):
    from syncfusion_amd.onset_loss import balanced_bce

    z, t, loss_ref, dz_ref = _loss_case(shape)
    runs = []
    for _ in range(2):
        zg = z.to(cuda).requires_grad_()
        loss = balanced_bce(zg, t.to(cuda))
        assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
        loss.backward()
        runs.append((loss.detach().clone(), zg.grad.clone()))
    # a non-unit upstream gradient that lives on the device
    zs = z.to(cuda).requires_grad_()
    (balanced_bce(zs, t.to(cuda)) * torch.tensor(UPSTREAM, device=cuda)).backward()
    # labels of another dtype are cast on the device
    loss_long = balanced_bce(z.to(cuda), t.to(cuda).long())
    torch.cuda.synchronize()
    e_loss = abs(float(runs[0][0]) - float(loss_ref)) / abs(float(loss_ref))
    e_dz = rel_l2(runs[0][1].cpu(), dz_ref)
    e_dzs = rel_l2(zs.grad.cpu(), UPSTREAM * dz_ref)
    print(f"balanced_bce {shape}: loss {e_loss:.2e}, dz {e_dz:.2e}, dz x {UPSTREAM} {e_dzs:.2e} (relative, vs fp64 BCLoss + autograd)")
    assert e_loss <= TOL and e_dz <= TOL and e_dzs <= TOL
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two calls on the same input differ"
    assert torch.equal(loss_long, runs[0][0])


@pytest.mark.autograd
@pytest.mark.parametrize("shape", [(2, 3), (16, 30), (33, 257)], ids=["2x3", "16x30", "33x257"])
def test_all_zero_labels_give_non_finite_loss_and_gradient(cuda, shape):
    from syncfusion_amd.onset_loss import balanced_bce

    z = torch.from_numpy(ref.grid_logits(np.random.default_rng(5), shape)).to(cuda).requires_grad_()
    loss = balanced_bce(z, torch.zeros(shape, device=cuda))
    loss.backward()
    torch.cuda.synchronize()
    assert not math.isfinite(float(loss))
    assert not bool(torch.isfinite(z.grad).any())


# ---- metrics ---------------------------------------------------------------------------------------------------------------------------------
METRIC_SHAPES = [(1, 1), (1, 2), (2, 3), (3, 30), (7, 37), (16, 30), (33, 257), (64, 64), (17, 241)]   # 64 x 64 / 17 x 241: the last size of
DENSITIES = [0.05, 0.3, 0.5, 0.9]                                                                       # the one-launch path and the first past it
HI, LO = 2.0, -2.0      # sigmoid 0.88 / 0.12


def _hand_cases():
    cases = {}
    # runs of length 1..5 at the row start and at the row end; the label count matches ceil(L / 2) in the first half of the rows only
    z = np.full((20, 12), LO, dtype=np.float32)
    t = np.zeros((20, 12), dtype=np.float32)
    for L in range(1, 6):
        for row, sl in ((2 * (L - 1), slice(0, L)), (2 * (L - 1) + 1, slice(12 - L, 12))):
            z[row, sl] = HI
            t[row, 5:5 + (L + 1) // 2] = 1.0
            z[10 + row, sl] = HI
            t[10 + row, 5:5 + L] = 1.0          # the unsuppressed count: a hit for L = 1 only
    cases["runs_at_row_edges"] = (z, t)
    # a row that ends in a prediction followed by a row that starts with one: two runs of one, not one run of two
    z = np.full((3, 4), LO, dtype=np.float32)
    z[0, 3] = z[1, 0] = z[1, 3] = z[2, 0] = HI
    t = np.zeros((3, 4), dtype=np.float32)
    t[0, 0] = t[1, 1] = t[1, 2] = t[2, 2] = 1.0
    cases["runs_do_not_join_across_rows"] = (z, t)
    rng = np.random.default_rng(77)
    cases["T1"] = (ref.grid_logits(rng, (9, 1)), np.array([[1], [0], [0], [1], [1], [0], [0], [0], [1]], dtype=np.float32))
    z = (rng.integers(128, 513, size=(5, 11)) / 64.0).astype(np.float32)             # every score above the threshold: 2 <= z <= 8
    cases["all_above_threshold"] = (z, ref.random_labels(rng, (5, 11), 0.4))
    cases["heavy_ties"] = (rng.choice(np.array([-1.0, 0.5, 2.0], dtype=np.float32), size=(6, 25)), ref.random_labels(rng, (6, 25), 0.5))
    z = ref.grid_logits(rng, (8, 30))
    sat = rng.random((8, 30)) < 0.4
    z[sat] = rng.choice(np.array([20.0, 25.0, 30.0], dtype=np.float32), size=int(sat.sum()))
    cases["saturated_group"] = (z, ref.random_labels(rng, (8, 30), 0.5))
    # b = 2: the first two negatives score low, every later negative scores far above the positives.  First-b subset: AP = 1; the last two
    # negatives instead (or any two of the later ones) would give AP = 1/2 * (1/3 + 2/4) = 0.42
    z = np.array([[1.0, -4.0, 2.0, -4.0], [8.0, 8.0, 8.0, 8.0]], dtype=np.float32)
    t = np.array([[1, 0, 1, 0], [0, 0, 0, 0]], dtype=np.float32)
    cases["subset_is_the_first_b"] = (z, t)
    z = ref.grid_logits(rng, (4, 9))
    cases["one_class_zeros"] = (z, np.zeros((4, 9), dtype=np.float32))
    cases["one_class_ones"] = (z, np.ones((4, 9), dtype=np.float32))
    return cases


def _random_cases():
    cases = {}
    for shape in METRIC_SHAPES:
        for d in DENSITIES:
            rng = np.random.default_rng(shape[0] * 1000 + shape[1] * 10 + int(d * 100))
            cases[f"{shape[0]}x{shape[1]}_d{d}"] = (ref.grid_logits(rng, shape), ref.random_labels(rng, shape, d))
    return cases


CASES = {**_random_cases(), **_hand_cases()}


@functools.lru_cache(maxsize=None)
def _metrics_ref(name):
    return ref.step_metrics_ref(*CASES[name])


def _same(a: float, b: float, tol: float = 0.0) -> bool:
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol


def test_hand_case_subset_choice_matters():
    """The case is built so that a wrong subset moves AP by more than 0.1 (checked on the helper: no device needed for this part)."""
    z, t = CASES["subset_is_the_first_b"]
    assert _metrics_ref("subset_is_the_first_b")["AP"] == 1.0
    s = ref.sigmoid32(z).reshape(-1)
    wrong = np.array([0, 2, 6, 7])
    assert abs(ref.average_precision(t.reshape(-1)[wrong].astype(np.float64), s[wrong]) - 1.0) > 0.1


@pytest.mark.parametrize("name", list(CASES), ids=list(CASES))
def test_step_metrics(cuda, name):
    from syncfusion_amd.module_onset import BCLoss
    from syncfusion_amd.onset_loss import DeviceBCLoss, step_metrics

    z, t = CASES[name]
    want = _metrics_ref(name)
    zg, tg = torch.from_numpy(z).to(cuda), torch.from_numpy(t).to(cuda)
    m = step_metrics(zg, tg)
    assert m.shape == (3,) and m.dtype == torch.float64 and m.device.type == "cuda"
    d = DeviceBCLoss().evaluate(zg, tg)
    assert set(d) == {"AP", "Acc", "OnsNumAcc"} and all(v.dim() == 0 and v.is_cuda for v in d.values())
    again = step_metrics(zg, tg)
    got = [float(v) for v in m.cpu()]
    print(f"step_metrics {name}: b = {want['b']}, AP {got[0]!r} (helper {want['AP']!r}), Acc {got[1]!r} ({want['Acc']!r}), "
          f"OnsNumAcc {got[2]!r} ({want['OnsNumAcc']!r})")
    assert _same(got[0], want["AP"], 1e-12), "AP"
    assert _same(got[1], want["Acc"]), "Acc"
    assert got[2] == want["OnsNumAcc"], "OnsNumAcc"
    assert torch.equal(m.cpu().view(torch.int64), again.cpu().view(torch.int64)), "two calls on the same input differ"
    assert all(_same(float(d[k]), got[i]) for i, k in enumerate(("AP", "Acc", "OnsNumAcc")))
    if want["b"] == 0:
        assert math.isnan(got[0]) and math.isnan(got[1])      # one class only: defined here, an IndexError in BCLoss.evaluate
    else:
        host = BCLoss().evaluate(zg, tg)                       # the reference's path, fed the same GPU tensors
        assert _same(host["AP"], got[0], 1e-12) and host["Acc"] == got[1] and host["OnsNumAcc"] == got[2], host


def test_step_metrics_other_label_dtypes_and_threshold(cuda):
    from syncfusion_amd.onset_loss import step_metrics

    z, t = CASES["16x30_d0.3"]
    zg, tg = torch.from_numpy(z).to(cuda), torch.from_numpy(t).to(cuda)
    base = step_metrics(zg, tg)
    assert torch.equal(step_metrics(zg, tg.long()), base) and torch.equal(step_metrics(zg, tg.bool()), base)
    want = ref.step_metrics_ref(z, t, threshold=0.5)          # sigmoid(0) = 0.5: grid logits equal to 0 sit ON the threshold (s > thr is false)
    got = [float(v) for v in step_metrics(zg, tg, threshold=0.5).cpu()]
    assert _same(got[0], want["AP"], 1e-12) and got[1] == want["Acc"] and got[2] == want["OnsNumAcc"]
    with pytest.raises(ValueError):
        step_metrics(zg.view(-1), tg.view(-1))
    with pytest.raises(TypeError):
        step_metrics(zg.double(), tg)


# ---- the step -------------------------------------------------------------------------------------------------------------------------------
def _hip_model(net, cuda, **kw):
    from syncfusion_amd import OnsetModel

    return OnsetModel(1e-3, 0.9, 0.999, 1e-8, 1e-2, net, loss="hip", **kw).to(cuda)


@pytest.mark.autograd
def test_training_step_does_not_synchronise(cuda):
    net = _seeded_net(7).to(cuda).train()
    model = _hip_model(net, cuda)
    g = torch.Generator().manual_seed(3)
    batch = {"frames": torch.randn(2, 3, 4, 32, 32, generator=g).to(cuda), "label": _labels(2, 4, 4).to(cuda)}
    model.training_step(batch, 0).backward()       # lazy initialisation (library load, workspace growth) outside the checked call
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=cuda).item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            loss = model.training_step(batch, 1)
            loss.backward()
            metrics = model.loss.last_metrics
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        pytest.skip("this torch build does not honour torch.cuda.set_sync_debug_mode('error'): .item() did not raise under it")
    torch.cuda.synchronize()
    assert math.isfinite(float(loss)) and metrics.shape == (3,) and metrics.is_cuda


@pytest.mark.autograd
@pytest.mark.parametrize("shape", [(2, 3, 4, 32, 32), (1, 3, 3, 24, 40), (2, 3, 5, 29, 35)], ids=["2x4x32x32", "N1_3x24x40", "odd_5x29x35"])
def test_onsetnet_train_step_hip_loss(cuda, shape, monkeypatch):
    """test_onsetnet_train_step with loss="hip": logits, loss and every gradient against the same fp64 oracle step, at the same gate."""
    N, _, T, H, W = shape
    net = _seeded_net(7)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(3))
    labels = _labels(N, T, 4)
    net = net.to(cuda).train()
    model = _hip_model(net, cuda)
    logits = net(x.to(cuda))                                   # Model.common_step, with the logits kept
    loss = model.loss(logits, labels.to(cuda))
    metrics = model.loss.evaluate(logits, labels.to(cuda))
    loss.backward()
    torch.cuda.synchronize()
    P, lref, loss_ref = _oracle_step(state, x, labels, monkeypatch)
    e_logits = rel_l2(logits.detach().cpu(), lref)
    e_loss = abs(float(loss.detach()) - float(loss_ref)) / abs(float(loss_ref))
    grads = []
    for k, p in net.named_parameters():
        assert p.grad is not None, f"{k}: no gradient"
        grads.append((k, rel_l2(p.grad.cpu(), P[k].grad)))
    wg = _worst(grads)
    print(f"onset train step, loss='hip' {shape}: logits {e_logits:.2e}, loss {e_loss:.2e}, worst gradient {wg[0]} {wg[1]:.2e}")
    assert e_logits <= NET_TOL and e_loss <= NET_TOL
    bad = [(k, e) for k, e in grads if not e <= NET_TOL]
    assert not bad, bad
    assert all(0.0 <= float(v) <= 1.0 for v in metrics.values())
