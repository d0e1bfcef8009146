"""VideoOnsetNet training on the HIP kernels (syncfusion_amd/onset_training.py, sf_op_vconv_* / sf_op_bn_train_*), against CPU autograd
in fp64: every convolution geometry of the net, BatchNorm3d in train mode (offset and constant channels), one whole training step at three
shapes (logits, BCLoss, every parameter gradient, every running buffer), determinism, the eval engine after AdamW steps, routing, and one
step at the reference's batch (16 x (3, 30, 112, 112)) against the same step on torch's own Conv3d / BatchNorm3d modules."""
from __future__ import annotations

import contextlib
import signal

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import numerics as nx
from helpers import rel_l2, seeded_state

pytestmark = [pytest.mark.gpu, pytest.mark.autograd]

TOL = 2e-5          # per-op gradients (the training tests' tolerance, tests/test_gpu_train.py)
NET_TOL = 1e-4      # whole-network step, per tensor
ONSET_FP32_TOL = 1e-4


def _rows(x: torch.Tensor, ld: int) -> torch.Tensor:
    """(N, C, T, H, W) -> channels-last rows (N*T*H*W, ld), zero padded."""
    N, Cc, T, H, W = x.shape
    r = torch.zeros(N * T * H * W, ld, dtype=x.dtype)
    r[:, :Cc] = x.permute(0, 2, 3, 4, 1).reshape(-1, Cc)
    return r


def _unrows(r: torch.Tensor, N: int, Cc: int, T: int, H: int, W: int) -> torch.Tensor:
    return r[:, :Cc].reshape(N, T, H, W, Cc).permute(0, 4, 1, 2, 3)


# (name, cin, cout, kernel, stride (h, w), padding, N, T, H, W): every geometry of the net, odd channel counts and frame sizes
CONV_CASES = [
    ("stem", 3, 45, (1, 7, 7), 2, (0, 3, 3), 2, 2, 15, 9),
    ("temporal45", 45, 64, (3, 1, 1), 1, (1, 0, 0), 2, 5, 7, 9),
    ("temporal_T1", 144, 64, (3, 1, 1), 1, (1, 0, 0), 1, 1, 9, 7),
    ("temporal921", 921, 512, (3, 1, 1), 1, (1, 0, 0), 1, 2, 3, 5),
    ("spatial_s1", 64, 144, (1, 3, 3), 1, (0, 1, 1), 2, 2, 9, 7),
    ("spatial_s1_460", 460, 256, (1, 3, 3), 1, (0, 1, 1), 1, 2, 7, 7),
    ("spatial_s2_230", 64, 230, (1, 3, 3), 2, (0, 1, 1), 2, 2, 15, 9),
    ("spatial_s2_921", 256, 921, (1, 3, 3), 2, (0, 1, 1), 1, 2, 7, 9),
    ("shortcut_s2", 128, 256, (1, 1, 1), 2, (0, 0, 0), 2, 5, 15, 7),
    ("shortcut_s2_odd", 230, 460, (1, 1, 1), 2, (0, 0, 0), 1, 2, 9, 15),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_vconv_forward_and_gradients(cuda, case):
    from syncfusion_amd.onset_training import conv_geometry, row_ld, vconv

    name, cin, cout, k, s, p, N, T, H, W = case
    conv = nn.Conv3d(cin, cout, k, stride=(1, s, s), padding=p, bias=False)
    g = torch.Generator().manual_seed(11)
    w = torch.randn(cout, cin, *k, generator=g) / (cin * k[0] * k[1] * k[2]) ** 0.5
    x = torch.randn(N, cin, T, H, W, generator=g)
    geo = conv_geometry(conv, N, T, H, W)
    Ho, Wo = geo.out_hw
    dy = torch.randn(N, cout, T, Ho, Wo, generator=g)
    # fp64 oracle
    xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
    yd = F.conv3d(xd, wd, None, stride=(1, s, s), padding=p)
    yd.backward(dy.double())
    # HIP
    xr = _rows(x, row_ld(cin)).to(cuda).requires_grad_()
    wg = w.to(cuda).requires_grad_()
    y = vconv(xr, wg, geo)
    y.backward(_rows(dy, row_ld(cout)).to(cuda))
    torch.cuda.synchronize()
    e_y = rel_l2(_unrows(y.detach().cpu(), N, cout, T, Ho, Wo), yd)
    e_dx = rel_l2(_unrows(xr.grad.cpu(), N, cin, T, H, W), xd.grad)
    e_dw = rel_l2(wg.grad.cpu(), wd.grad)
    print(f"vconv {name}: y {e_y:.2e}, dx {e_dx:.2e}, dw {e_dw:.2e}")
    assert float(y.detach()[:, cout:].abs().max() if row_ld(cout) > cout else 0.0) == 0.0, "padding columns of y must be zero"
    assert float(xr.grad[:, cin:].abs().max() if row_ld(cin) > cin else 0.0) == 0.0, "padding columns of dx must be zero"
    assert e_y <= TOL and e_dx <= TOL and e_dw <= TOL, (e_y, e_dx, e_dw)


@pytest.mark.parametrize("regime", ["plain", "offset:1000", "const"])
@pytest.mark.parametrize("relu,with_res", [(True, False), (False, False), (True, True)])
def test_batchnorm_train(cuda, regime, relu, with_res):
    from syncfusion_amd.onset_training import batch_norm_train

    N, Cc, T, H, W = 2, 45, 3, 5, 7
    g = torch.Generator().manual_seed(5)
    mu = torch.randn(Cc, generator=g)
    sd = torch.rand(Cc, generator=g) + 0.5
    if regime.startswith("offset"):
        mu = mu.sign() * float(regime.split(":")[1]) * sd       # mean / spread = 1000
    x = mu.view(1, Cc, 1, 1, 1) + sd.view(1, Cc, 1, 1, 1) * torch.randn(N, Cc, T, H, W, generator=g)
    x[:, 7] = 3.25                                               # one constant channel in every regime
    if regime == "const":
        x[:, 20] = -1.5e3
    res = torch.randn(N, Cc, T, H, W, generator=g) if with_res else None
    dy = torch.randn(N, Cc, T, H, W, generator=g)
    bn = nn.BatchNorm3d(Cc)
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.2 * torch.randn(Cc, generator=g))
        bn.bias.copy_(0.1 * torch.randn(Cc, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(Cc, generator=g))
        bn.running_var.copy_(torch.rand(Cc, generator=g) + 0.5)
    # fp64 oracle on clones of the buffers
    rm, rv = bn.running_mean.double().clone(), bn.running_var.double().clone()
    xd = x.double().requires_grad_()
    gd, bd = bn.weight.detach().double().requires_grad_(), bn.bias.detach().double().requires_grad_()
    resd = res.double().requires_grad_() if with_res else None
    z = F.batch_norm(xd, rm, rv, gd, bd, training=True, momentum=0.1, eps=1e-5)
    if with_res:
        z = z + resd
    yd = F.relu(z) if relu else z
    mean_d = x.double().mean(dim=(0, 2, 3, 4))
    invstd_d = 1.0 / (x.double().var(dim=(0, 2, 3, 4), unbiased=False) + 1e-5).sqrt()
    # HIP
    bn = bn.to(cuda)
    ld = 64
    xr = _rows(x, ld).to(cuda).requires_grad_()
    rr = _rows(res, ld).to(cuda).requires_grad_() if with_res else None
    y = batch_norm_train(xr, bn, rr, relu)
    saved = y.grad_fn.saved_tensors    # (x, y or None, gamma, mean, invstd)
    y.backward(_rows(dy, ld).to(cuda))
    torch.cuda.synchronize()
    # the ReLU mask is part of the forward output: the oracle's backward takes the kernel's (an element within fp32 rounding of 0 may
    # fall either side; the output check above covers the values themselves)
    mask = (_unrows(y.detach().cpu(), N, Cc, T, H, W) > 0).double() if relu else 1.0
    z.backward(dy.double() * mask)
    ratio = float((mu.abs() / sd).max())
    gate = nx.offset_gate(TOL, ratio) if regime.startswith("offset") else TOL
    sh = (N, Cc, T, H, W)
    nx.check_close(_unrows(y.detach().cpu(), *sh), yd, gate, f"bn y {regime}")
    assert float(y.detach()[:, Cc:].abs().max()) == 0.0
    nx.check_close(saved[3].cpu(), mean_d, max(TOL, 8 * nx.U24), f"bn saved mean {regime}", dims=("channel",))
    nx.check_close(saved[4].cpu(), invstd_d, gate, f"bn saved invstd {regime}", dims=("channel",))
    nx.check_close(bn.running_mean.cpu(), rm, max(TOL, 8 * nx.U24), f"bn running_mean {regime}", dims=("channel",))
    nx.check_close(bn.running_var.cpu(), rv, gate, f"bn running_var {regime}", dims=("channel",))
    assert int(bn.num_batches_tracked) == 1
    nx.check_close(_unrows(xr.grad.cpu(), *sh), xd.grad, gate, f"bn dx {regime}")
    nx.check_close(bn.weight.grad.cpu(), gd.grad, gate, f"bn dgamma {regime}", dims=("channel",))
    nx.check_close(bn.bias.grad.cpu(), bd.grad, TOL, f"bn dbeta {regime}", dims=("channel",))
    if with_res:
        nx.check_close(_unrows(rr.grad.cpu(), *sh), resd.grad, TOL, f"bn dres {regime}")


# ---------------------------------------------------------------------------------------------------------------------------------
# whole network
# ---------------------------------------------------------------------------------------------------------------------------------
def _seeded_net(seed: int = 7):
    from syncfusion_amd.onset_net import VideoOnsetNet

    net = VideoOnsetNet(False)
    net.load_state_dict(seeded_state(net, seed))
    return net


def _labels(N: int, T: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    lab = (torch.rand(N, T, generator=g) < 0.3).float()
    lab[0, 0] = 1.0   # at least one positive and one negative
    lab[-1, -1] = 0.0
    return lab


def _oracle_step(state, x, labels, monkeypatch):
    """onsetnet_ref.onsetnet_forward with train-mode BatchNorm on cloned running buffers, fp64, + BCLoss + backward."""
    from oracle import onsetnet_ref
    from syncfusion_amd.module_onset import BCLoss

    P = {k: v.double().clone().requires_grad_(not k.endswith(("running_mean", "running_var", "num_batches_tracked")) and v.is_floating_point())
         for k, v in state.items()}

    def _bn(P_, pre, x_):
        return F.batch_norm(x_, P_[pre + ".running_mean"], P_[pre + ".running_var"], P_[pre + ".weight"], P_[pre + ".bias"], training=True,
                            momentum=0.1, eps=1e-5)

    monkeypatch.setattr(onsetnet_ref, "_bn", _bn)
    logits = onsetnet_ref.onsetnet_forward(P, x.double())
    loss = BCLoss()(logits, labels.double())
    loss.backward()
    return P, logits.detach(), loss.detach()


def _worst(items):
    return max(items, key=lambda kv: kv[1])


@pytest.mark.parametrize("shape", [(2, 3, 4, 32, 32), (1, 3, 3, 24, 40), (2, 3, 5, 29, 35)], ids=["2x4x32x32", "N1_3x24x40", "odd_5x29x35"])
def test_onsetnet_train_step(cuda, shape, monkeypatch):
    from syncfusion_amd.module_onset import BCLoss

    N, _, T, H, W = shape
    net = _seeded_net(7)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, generator=g)
    labels = _labels(N, T, 4)
    net = net.to(cuda).train()
    logits = net(x.to(cuda))
    assert logits.shape == (N, T) and logits.requires_grad
    loss = BCLoss()(logits, labels.to(cuda))
    loss.backward()
    torch.cuda.synchronize()
    P, lref, loss_ref = _oracle_step(state, x, labels, monkeypatch)
    e_logits = rel_l2(logits.detach().cpu(), lref)
    e_loss = abs(float(loss.detach()) - float(loss_ref)) / abs(float(loss_ref))
    grads, bufs = [], []
    for k, p in net.named_parameters():
        assert p.grad is not None, f"{k}: no gradient"
        grads.append((k, rel_l2(p.grad.cpu(), P[k].grad)))
    for k, b in net.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == 1, k
        else:
            bufs.append((k, rel_l2(b.cpu(), P[k].detach())))
    wg, wb = _worst(grads), _worst(bufs)
    print(f"onset train step {shape}: logits {e_logits:.2e}, loss {e_loss:.2e}, worst gradient {wg[0]} {wg[1]:.2e}, "
          f"worst running buffer {wb[0]} {wb[1]:.2e}")
    assert e_logits <= NET_TOL and e_loss <= NET_TOL
    bad = [(k, e) for k, e in grads + bufs if not e <= NET_TOL]
    assert not bad, bad


def test_onsetnet_backward_deterministic(cuda):
    from syncfusion_amd.module_onset import BCLoss

    net = _seeded_net(9).to(cuda).train()
    x = torch.randn(2, 3, 4, 32, 32, generator=torch.Generator().manual_seed(1)).to(cuda)
    labels = _labels(2, 4, 2).to(cuda)
    runs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        BCLoss()(net(x), labels).backward()
        runs.append({k: p.grad.clone() for k, p in net.named_parameters()})
    torch.cuda.synchronize()
    diff = [k for k in runs[0] if not torch.equal(runs[0][k], runs[1][k])]
    assert not diff, f"gradients differ between two identical backward passes: {diff[:5]}"


def _batch(N, T, H, W, seed, cuda):
    g = torch.Generator().manual_seed(seed)
    return {"frames": torch.randn(N, 3, T, H, W, generator=g).to(cuda), "label": _labels(N, T, seed + 1).to(cuda)}


def test_eval_engine_follows_training(cuda):
    from oracle import onsetnet_ref
    from syncfusion_amd import OnsetModel

    net = _seeded_net(7).to(cuda)
    model = OnsetModel(1e-3, 0.9, 0.999, 1e-8, 1e-2, net).to(cuda)
    opt = model.configure_optimizers()
    x = torch.randn(2, 3, 4, 32, 32, generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        before = net.eval()(x.to(cuda)).cpu()      # builds the engine on the initial weights
    net.train()
    batch = _batch(2, 4, 32, 32, 21, cuda)
    for i in range(3):
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(batch, i)
        loss.backward()
        opt.step()
    with torch.no_grad():
        y = net.eval()(x.to(cuda)).cpu()
        ref = onsetnet_ref.onsetnet_forward({k: v.detach().float().cpu() for k, v in net.state_dict().items()}, x)
    e = rel_l2(y, ref)
    print(f"eval engine after 3 AdamW steps: rel-L2 {e:.2e} (moved {rel_l2(before, ref):.2e} from the initial logits)")
    assert int(net.net.model.stem[1].num_batches_tracked) == 3
    assert rel_l2(before, ref) > 10 * ONSET_FP32_TOL, "the steps did not change the logits"
    assert e < ONSET_FP32_TOL


def test_loss_goes_down(cuda):
    from syncfusion_amd import OnsetModel

    net = _seeded_net(12).to(cuda).train()
    model = OnsetModel(1e-3, 0.9, 0.999, 1e-8, 0.0, net).to(cuda)
    opt = model.configure_optimizers()
    batch = _batch(2, 4, 32, 32, 31, cuda)
    losses = []
    for i in range(6):
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(batch, i)
        assert loss.requires_grad and loss.grad_fn is not None
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("BCLoss over 6 steps:", [f"{v:.4f}" for v in losses])
    assert losses[-1] < 0.9 * losses[0], losses


def test_routing(cuda):
    from syncfusion_amd._lib import SyncFusionAmdError

    net = _seeded_net(7).to(cuda).eval()
    x = torch.randn(2, 3, 4, 32, 32, generator=torch.Generator().manual_seed(2)).to(cuda)
    y_grad = net(x)
    with torch.no_grad():
        y_nograd = net(x)
        y_engine = net._get_engine().forward(x)
    assert not y_grad.requires_grad
    assert torch.equal(y_grad, y_engine) and torch.equal(y_nograd, y_engine)
    net.train()
    with torch.no_grad(), pytest.raises(RuntimeError):
        net(x)
    with pytest.raises(SyncFusionAmdError):
        net(x.cpu())
    with pytest.raises(ValueError):
        net(torch.zeros(1, 4, 4, 32, 32, device=cuda))


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's batch, once, against torch's own modules (MIOpen)
# ---------------------------------------------------------------------------------------------------------------------------------
def torch_modules_forward(net, x):
    """main/onset_net.py:57-63 on the nn.Conv3d / nn.BatchNorm3d modules that hold the parameters (train-mode BatchNorm)."""
    m = net.net.model
    h = m.stem(x)
    for name in ("layer1", "layer2", "layer3", "layer4"):
        for blk in getattr(m, name):
            res = h if blk.downsample is None else blk.downsample(h)
            h = F.relu(blk.conv2(blk.conv1(h)) + res)
    h = h.mean(dim=(3, 4)).transpose(-1, -2)
    return net.fc(h).squeeze(-1)


@contextlib.contextmanager
def _deadline(seconds: int):
    def _raise(*_):
        raise TimeoutError(f"reference-batch step exceeded {seconds} s")

    old = signal.signal(signal.SIGALRM, _raise)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def test_reference_batch_step_vs_torch_modules(cuda):
    """One step at 16 x (3, 30, 112, 112) (cfg/data/data-onset-greatesthit.yaml: 2 s at 15 fps).  Both sides run fp32 on this GPU; neither
    is an fp64 reference (the fp64 checks are test_onsetnet_train_step's, at 1e-4 per tensor on small shapes).  Gates: 1e-3 rel-L2 for
    the logits and the loss; GRAD_GATE for the sampled gradients (the stem, a layer-3 mid convolution, the last BatchNorm, the head).  The
    gradients of the early layers pass back through up to 34 train-mode BatchNorms, whose backward subtracts per-channel means over
    1.5 M rows at this batch: two fp32 implementations with different summation orders measured 1.6e-2 (stem weight) and 7.4e-3 (last
    BatchNorm weight) apart, the head 6.5e-6.  Which side is closer to fp64 at this size is not measured (no fp64 convolution on the GPU)."""
    GRAD_GATE = 5e-2
    import copy

    from syncfusion_amd.module_onset import BCLoss

    with _deadline(600):
        net = _seeded_net(7).to(cuda).train()
        ref_net = copy.deepcopy(net)
        g = torch.Generator().manual_seed(17)
        x = torch.randn(16, 3, 30, 112, 112, generator=g).to(cuda)
        labels = _labels(16, 30, 18).to(cuda)
        loss = BCLoss()(logits := net(x), labels)
        loss.backward()
        loss_t = BCLoss()(logits_t := torch_modules_forward(ref_net, x), labels)
        loss_t.backward()
        torch.cuda.synchronize()
    e_l = rel_l2(logits.detach(), logits_t.detach())
    e_loss = abs(float(loss) - float(loss_t)) / abs(float(loss_t))
    pick = ["net.model.stem.0.weight", "net.model.layer3.1.conv1.0.0.weight", "net.model.layer4.1.conv2.1.weight", "fc.0.weight"]
    mine, theirs = dict(net.named_parameters()), dict(ref_net.named_parameters())
    errs = {k: rel_l2(mine[k].grad, theirs[k].grad) for k in pick}
    print(f"reference batch: logits {e_l:.2e}, loss {e_loss:.2e}, gradients {errs}")
    assert e_l < 1e-3 and e_loss < 1e-3 and all(e < GRAD_GATE for e in errs.values()), (e_l, e_loss, errs)
