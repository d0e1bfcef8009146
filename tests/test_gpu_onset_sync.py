"""Cross-rank BatchNorm of the onset net's training step (syncfusion_amd/onset_training.py _BNSyncTrain, sf_op_bn_sync_*).

Multi-rank cases run as tests/test_gpu_dist.py does: spawned processes, gloo rendezvous on a free port, every rank on cuda:0.  The oracle
of every multi-rank case is ONE fp64 CPU pass over the concatenated batch with train-mode BatchNorm and the objective
(1 / world) * sum_r loss_r(shard r): its gradients are what synchronised BatchNorm plus gradient averaging must produce, for even and
uneven shards and with BCLoss's per-shard pos_weight.

Measured on an MI355X (gates: TOL = 2e-5 per op, numerics.offset_gate = 4.8e-4 at offset:1000, NET_TOL = 1e-4 per tensor of a whole step):
  op level       plain / const, worst case: y 8.5e-08, dx 7.5e-08, dres 0 (exact), sum of local dgamma 1.4e-07, sum of local dbeta 1.1e-07;
                 offset:1000: y 3.1e-05, dx 1.0e-07, sum of local dgamma 5.2e-05
  two-rank step  2+2: logits 1.2e-05, loss 7.7e-07, worst gradient 1.7e-05, worst running buffer 7.5e-07
                 3+1: logits 1.6e-05, loss 1.6e-06, worst gradient 1.9e-05, worst running buffer 7.1e-07
                 2+1 of (3, 3, 5, 29, 35): logits 2.2e-05, loss 1.6e-06, worst gradient 1.7e-05, worst running buffer 6.4e-07
                 (the single-rank step on the full batch: logits 1.4e-05, worst running buffer 7.0e-07)
  three data-parallel AdamW steps, then eval(): engine against the oracle 1.3e-07
  split-phase step with RCCL carrying the 74 gathers (one rank) against the plain path: 0 (bit-equal)
"""
from __future__ import annotations

import hashlib
import os
import queue
import socket
import sys
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn
import torch.nn.functional as F

import numerics as nx
from helpers import ROOT, rel_l2, seeded_state

pytestmark = [pytest.mark.gpu, pytest.mark.autograd]

TOL = 2e-5          # per-op gradients (tests/test_gpu_onset_train.py)
NET_TOL = 1e-4      # whole-network step, per tensor


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. op level, one process: the split-phase calls on row ranges of one tensor, "gathering" by hand
# ---------------------------------------------------------------------------------------------------------------------------------
def _rows(x: torch.Tensor, ld: int) -> torch.Tensor:
    N, Cc, T, H, W = x.shape
    r = torch.zeros(N * T * H * W, ld, dtype=x.dtype)
    r[:, :Cc] = x.permute(0, 2, 3, 4, 1).reshape(-1, Cc)
    return r


def _unrows(r: torch.Tensor, N: int, Cc: int, T: int, H: int, W: int) -> torch.Tensor:
    return r[:, :Cc].reshape(N, T, H, W, Cc).permute(0, 4, 1, 2, 3)


def _split_phase_bn(cuda, xr, rr, dyr, spans, Cc, gamma, beta, rm0, rv0, relu, eps=1e-5, momentum=0.1):
    """Every 'rank' owns the rows [lo, hi) of xr; returns the concatenated y / dx / dres, the per-rank (mean, invstd, running buffers, nbt)
    and the per-rank local dgamma / dbeta."""
    from syncfusion_amd import _lib

    lib = _lib.load()
    st = _lib.stream_ptr(cuda)
    ld = xr.shape[1]
    world = len(spans)
    counts = torch.tensor([hi - lo for lo, hi in spans], dtype=torch.int64).to(cuda)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731

    def ws_for(rows):
        n = lib.sf_op_bn_sync_workspace_bytes(rows, Cc)
        assert n > 0
        return torch.empty(n, dtype=torch.uint8, device=cuda)

    xs = [xr[lo:hi].contiguous() for lo, hi in spans]
    rs = [rr[lo:hi].contiguous() if rr is not None else None for lo, hi in spans]
    dys = [dyr[lo:hi].contiguous() for lo, hi in spans]
    table = torch.empty(world, Cc, 2, dtype=torch.float32, device=cuda)
    for r, x in enumerate(xs):
        ws = ws_for(x.shape[0])
        _lib.check(lib.sf_op_bn_sync_stats(x.data_ptr(), x.shape[0], Cc, ld, table[r].data_ptr(), ws.data_ptr(), ws.numel(), st), "sf_op_bn_sync_stats")
    ys, per_rank = [], []
    for r, x in enumerate(xs):
        ws = ws_for(x.shape[0])
        y = torch.empty_like(x)
        mean, invstd = torch.empty(Cc, device=cuda), torch.empty(Cc, device=cuda)
        rm, rv, nbt = rm0.clone().to(cuda), rv0.clone().to(cuda), torch.zeros((), dtype=torch.int64, device=cuda)
        _lib.check(lib.sf_op_bn_sync_fwd_apply(x.data_ptr(), ptr(rs[r]), x.shape[0], Cc, ld, table.data_ptr(), counts.data_ptr(), world, gamma.data_ptr(),
                                               beta.data_ptr(), eps, momentum, rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), int(relu), y.data_ptr(),
                                               mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), ws.numel(), st), "sf_op_bn_sync_fwd_apply")
        ys.append(y)
        per_rank.append((mean, invstd, rm, rv, nbt))
    sums = torch.empty(world, Cc, 2, dtype=torch.float32, device=cuda)
    dgs, dbs = [], []
    for r, x in enumerate(xs):
        ws = ws_for(x.shape[0])
        dg, db = torch.empty(Cc, device=cuda), torch.empty(Cc, device=cuda)
        mean, invstd = per_rank[r][0], per_rank[r][1]
        _lib.check(lib.sf_op_bn_sync_bwd_sums(x.data_ptr(), ptr(ys[r]) if relu else None, dys[r].data_ptr(), x.shape[0], Cc, ld, mean.data_ptr(),
                                              invstd.data_ptr(), sums[r].data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), st),
                   "sf_op_bn_sync_bwd_sums")
        dgs.append(dg)
        dbs.append(db)
    dxs, drs = [], []
    for r, x in enumerate(xs):
        ws = ws_for(x.shape[0])
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if rr is not None else None
        mean, invstd = per_rank[r][0], per_rank[r][1]
        _lib.check(lib.sf_op_bn_sync_bwd_apply(x.data_ptr(), ptr(ys[r]) if relu else None, dys[r].data_ptr(), x.shape[0], Cc, ld, sums.data_ptr(),
                                               counts.data_ptr(), world, gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(), dx.data_ptr(), ptr(dres),
                                               ws.data_ptr(), ws.numel(), st), "sf_op_bn_sync_bwd_apply")
        dxs.append(dx)
        drs.append(dres)
    torch.cuda.synchronize()
    return torch.cat(ys), torch.cat(dxs), (torch.cat(drs) if rr is not None else None), per_rank, dgs, dbs


# rows = 2 * 3 * 5 * 7 = 210: two even ranges; three uneven ranges, the last of a single row
SPLITS = {"2even": [(0, 105), (105, 210)], "3uneven_1row": [(0, 150), (150, 209), (209, 210)]}


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("regime", ["plain", "offset:1000", "const"])
@pytest.mark.parametrize("relu,with_res", [(True, False), (False, False), (True, True)])
def test_split_phase_batchnorm_ops(cuda, regime, relu, with_res, split):
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
    gamma = 1.0 + 0.2 * torch.randn(Cc, generator=g)
    beta = 0.1 * torch.randn(Cc, generator=g)
    rm0 = 0.1 * torch.randn(Cc, generator=g)
    rv0 = torch.rand(Cc, generator=g) + 0.5
    # fp64 oracle: F.batch_norm on the WHOLE tensor
    rm, rv = rm0.double().clone(), rv0.double().clone()
    xd = x.double().requires_grad_()
    gd, bd = gamma.double().requires_grad_(), beta.double().requires_grad_()
    resd = res.double().requires_grad_() if with_res else None
    z = F.batch_norm(xd, rm, rv, gd, bd, training=True, momentum=0.1, eps=1e-5)
    if with_res:
        z = z + resd
    yd = F.relu(z) if relu else z
    mean_d = x.double().mean(dim=(0, 2, 3, 4))
    invstd_d = 1.0 / (x.double().var(dim=(0, 2, 3, 4), unbiased=False) + 1e-5).sqrt()
    # HIP, split phases
    ld = 64
    y, dx, dres, per_rank, dgs, dbs = _split_phase_bn(cuda, _rows(x, ld).to(cuda), _rows(res, ld).to(cuda) if with_res else None, _rows(dy, ld).to(cuda),
                                                      SPLITS[split], Cc, gamma.to(cuda), beta.to(cuda), rm0, rv0, relu)
    # the ReLU mask is part of the forward output: the oracle's backward takes the kernel's (as test_batchnorm_train does)
    mask = (_unrows(y.cpu(), N, Cc, T, H, W) > 0).double() if relu else 1.0
    z.backward(dy.double() * mask)
    ratio = float((mu.abs() / sd).max())
    gate = nx.offset_gate(TOL, ratio) if regime.startswith("offset") else TOL
    sh = (N, Cc, T, H, W)
    e_y = nx.check_close(_unrows(y.cpu(), *sh), yd, gate, f"sync bn y {regime}")
    assert float(y[:, Cc:].abs().max()) == 0.0 and float(dx[:, Cc:].abs().max()) == 0.0, "padding columns must be zero"
    mean0, invstd0, rm_0, rv_0, _ = per_rank[0]
    for r, (mean, invstd, rm_r, rv_r, nbt) in enumerate(per_rank):
        assert int(nbt) == 1
        # identical input in identical order: identical bits on every rank
        assert torch.equal(mean, mean0) and torch.equal(invstd, invstd0) and torch.equal(rm_r, rm_0) and torch.equal(rv_r, rv_0), f"rank {r} differs"
    nx.check_close(mean0.cpu(), mean_d, max(TOL, 8 * nx.U24), f"sync bn saved mean {regime}", dims=("channel",))
    nx.check_close(invstd0.cpu(), invstd_d, gate, f"sync bn saved invstd {regime}", dims=("channel",))
    nx.check_close(rm_0.cpu(), rm, max(TOL, 8 * nx.U24), f"sync bn running_mean {regime}", dims=("channel",))
    nx.check_close(rv_0.cpu(), rv, gate, f"sync bn running_var {regime}", dims=("channel",))
    e_dx = nx.check_close(_unrows(dx.cpu(), *sh), xd.grad, gate, f"sync bn dx {regime}")
    # dgamma / dbeta are LOCAL sums (torch.nn.SyncBatchNorm): their sum over the ranks is the full-batch gradient
    e_dg = nx.check_close(torch.stack(dgs).double().sum(0).cpu(), gd.grad, gate, f"sync bn sum of local dgamma {regime}", dims=("channel",))
    e_db = nx.check_close(torch.stack(dbs).double().sum(0).cpu(), bd.grad, TOL, f"sync bn sum of local dbeta {regime}", dims=("channel",))
    e_dr = nx.check_close(_unrows(dres.cpu(), *sh), resd.grad, TOL, f"sync bn dres {regime}") if with_res else 0.0
    print(f"split-phase bn {regime} relu={relu} res={with_res} {split}: y {e_y:.2e}, dx {e_dx:.2e}, dres {e_dr:.2e}, dgamma {e_dg:.2e}, "
          f"dbeta {e_db:.2e} (gate {gate:.1e})")


# ---------------------------------------------------------------------------------------------------------------------------------
# multi-rank machinery
# ---------------------------------------------------------------------------------------------------------------------------------
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(target, world: int, args: tuple, seconds: float):
    """Start `world` ranks, return their results by rank.  A worker that dies (non-zero exit) fails the test at once; no retries."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    out, deadline = {}, time.monotonic() + seconds
    try:
        while len(out) < world:
            try:
                rank, val = q.get(timeout=1.0)
                out[rank] = val
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead, f"worker exit codes {dead}"
                assert time.monotonic() < deadline, "workers did not answer in time"
        for p in procs:
            p.join(60)
            assert p.exitcode == 0, p.exitcode
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return out


def _init(rank: int, world: int, port: int, backend: str = "gloo"):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group(backend, rank=rank, world_size=world)


def _seeded_net(seed: int = 7):
    from syncfusion_amd.onset_net import VideoOnsetNet

    net = VideoOnsetNet(False)
    net.load_state_dict(seeded_state(net, seed))
    return net


def _labels(N: int, T: int, seed: int) -> torch.Tensor:
    """Every clip holds a positive and a negative frame, so that every shard's pos_weight is finite."""
    lab = (torch.rand(N, T, generator=torch.Generator().manual_seed(seed)) < 0.3).float()
    lab[:, 0] = 1.0
    lab[:, -1] = 0.0
    return lab


def _data(shape, seed_x: int = 3, seed_l: int = 4):
    N, _, T, _, _ = shape
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed_x)), _labels(N, T, seed_l)


def _spans(sizes):
    out, lo = [], 0
    for n in sizes:
        out.append((lo, lo + n))
        lo += n
    return out


def _digest(tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _hip_step(net, x, labels, cuda):
    from syncfusion_amd.module_onset import BCLoss

    net.zero_grad(set_to_none=True)
    logits = net(x.to(cuda))
    loss = BCLoss()(logits, labels.to(cuda))
    loss.backward()
    return logits.detach(), loss.detach()


def _step_worker(rank: int, world: int, port: int, q, shape, sizes, outdir: str):
    """One data-parallel step on this rank's shard, twice from the same weights (the second run is the determinism check)."""
    _init(rank, world, port)
    try:
        from syncfusion_amd import allreduce_gradients
        from syncfusion_amd import onset_training as ot

        cuda = torch.device("cuda:0")
        x, labels = _data(shape)
        lo, hi = _spans(sizes)[rank]
        runs, masks = [], []
        real = ot.batch_norm_train_sync

        def recording(x_, bn, sg, res=None, relu=False):
            y = real(x_, bn, sg, res, relu)
            if relu:
                masks.append((y.detach()[:, :bn.num_features] > 0).cpu())
            return y

        for i in range(2):
            ot.batch_norm_train_sync = recording if i == 0 else real    # the first run also records every ReLU mask (see _oracle_dp_step)
            net = nn.SyncBatchNorm.convert_sync_batchnorm(_seeded_net(7)).to(cuda).train()
            logits, loss = _hip_step(net, x[lo:hi], labels[lo:hi], cuda)
            calls = allreduce_gradients(net)
            torch.cuda.synchronize()
            assert calls >= 1
            runs.append({"logits": logits.cpu(), "loss": loss.cpu(), "grads": {k: p.grad.cpu() for k, p in net.named_parameters()},
                         "buffers": {k: b.cpu() for k, b in net.named_buffers()}})
        first, second = runs
        out = {"logits": first["logits"], "loss": first["loss"], "buffers": first["buffers"], "relu_masks": masks,
               "grad_digest": _digest(first["grads"].values()), "grad_digest_second_run": _digest(second["grads"].values()),
               "grads_differ_second_run": [k for k in first["grads"] if not torch.equal(first["grads"][k], second["grads"][k])]}
        if rank == 0:
            out["grads"] = first["grads"]
        torch.save(out, os.path.join(outdir, f"rank{rank}.pt"))
        q.put((rank, "ok"))
    finally:
        dist.destroy_process_group()


_STEP_CASES = {"2+2": ((4, 3, 4, 32, 32), (2, 2)), "3+1": ((4, 3, 4, 32, 32), (3, 1)), "odd_2+1": ((3, 3, 5, 29, 35), (2, 1))}
_step_cache: dict = {}


def _two_rank_step(case: str, tmp_path_factory):
    """The spawned two-rank step of `case`, run once per session and shared by the tests that read different parts of its result."""
    if case not in _step_cache:
        shape, sizes = _STEP_CASES[case]
        outdir = str(tmp_path_factory.mktemp("sync_step"))
        _spawn(_step_worker, len(sizes), (shape, sizes, outdir), 500)
        _step_cache[case] = [torch.load(os.path.join(outdir, f"rank{r}.pt")) for r in range(len(sizes))]
    return _step_cache[case]


KINK_BAND = NET_TOL  # in units of the activation's rms: what the forward may misplace within its own gate (NET_TOL per tensor)


class _KinkAwareF:
    """torch.nn.functional for the oracle, with one change: a ReLU input within KINK_BAND of zero takes the side the kernels took.

    ReLU has no derivative at zero, and an fp32 forward cannot place an element that the fp64 pass puts within its rounding error of zero:
    the gradient there is not defined to fp32 resolution.  The mask is part of the forward output, so the oracle's backward takes the
    kernels' mask for those elements -- the convention of test_batchnorm_train -- and ONLY for those: everywhere else the masks must agree.
    At 4 clips the net has 3 M ReLU inputs and the fp64 pass alone puts several within 4e-7 rms of zero; one flipped element of the last
    block is 1 % of that layer's bias gradient and 2 % of the stem's weight gradient (measured)."""

    def __init__(self, masks):
        self.masks, self.i, self.taken, self.flipped = masks, 0, 0, 0

    def __getattr__(self, name):
        return getattr(F, name)

    def relu(self, z, inplace=False):
        if self.masks is None or self.i >= len(self.masks) or z.dim() != 5:
            return F.relu(z)
        N, Cc, T, H, W = z.shape
        m = self.masks[self.i].reshape(N, T, H, W, Cc).permute(0, 4, 1, 2, 3)
        self.i += 1
        own = z.detach() > 0
        near = z.detach().abs() <= KINK_BAND * z.detach().pow(2).mean().sqrt()
        assert bool((m == own)[~near].all()), f"ReLU {self.i}: the kernels' mask differs from the oracle's outside the band around zero"
        self.taken += int(near.sum())
        self.flipped += int((m != own)[near].sum())
        return z * torch.where(near, m, own).to(z.dtype)


def _oracle_dp_step(state, x, labels, sizes, monkeypatch, masks=None):
    """ONE fp64 CPU pass over the concatenated batch with train-mode BatchNorm (oracle/onsetnet_ref.py), objective
    (1 / world) * sum_r BCLoss(shard r) -- BCLoss computes its pos_weight per shard, as every rank does.  `masks`: the kernels' ReLU masks in
    call order, (rows, C) each over the concatenated batch (see _KinkAwareF)."""
    from oracle import onsetnet_ref
    from syncfusion_amd.module_onset import BCLoss

    P = {k: v.double().clone().requires_grad_(not k.endswith(("running_mean", "running_var", "num_batches_tracked")) and v.is_floating_point())
         for k, v in state.items()}

    def _bn(P_, pre, x_):
        return F.batch_norm(x_, P_[pre + ".running_mean"], P_[pre + ".running_var"], P_[pre + ".weight"], P_[pre + ".bias"], training=True,
                            momentum=0.1, eps=1e-5)

    kf = _KinkAwareF(masks)
    monkeypatch.setattr(onsetnet_ref, "_bn", _bn)
    monkeypatch.setattr(onsetnet_ref, "F", kf)
    logits = onsetnet_ref.onsetnet_forward(P, x.double())
    assert masks is None or kf.i == len(masks) == 34
    losses = [BCLoss()(logits[lo:hi], labels[lo:hi].double()) for lo, hi in _spans(sizes)]
    sum(losses).div(len(sizes)).backward()
    print(f"  oracle: {kf.taken} ReLU inputs within {KINK_BAND:g} rms of zero took the kernels' side, {kf.flipped} of them against the fp64 sign")
    return P, logits.detach(), [l_.detach() for l_ in losses]


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. two ranks, whole step, against the fp64 oracle of the concatenated batch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize("case", list(_STEP_CASES))
def test_two_rank_step_matches_full_batch_oracle(cuda, case, monkeypatch, tmp_path_factory):
    shape, sizes = _STEP_CASES[case]
    ranks = _two_rank_step(case, tmp_path_factory)
    x, labels = _data(shape)
    state = seeded_state(_seeded_net(7), 7)
    masks = [torch.cat(ms) for ms in zip(*(r["relu_masks"] for r in ranks))]      # rank order = clip order
    P, lref, losses_ref = _oracle_dp_step(state, x, labels, sizes, monkeypatch, masks)
    logits = torch.cat([r["logits"] for r in ranks])
    e_logits = rel_l2(logits, lref)
    e_loss = max(abs(float(r["loss"]) - float(lr)) / abs(float(lr)) for r, lr in zip(ranks, losses_ref))
    grads = [(k, rel_l2(g_, P[k].grad)) for k, g_ in ranks[0]["grads"].items()]
    bufs = []
    for k, b in ranks[0]["buffers"].items():
        if k.endswith("num_batches_tracked"):
            assert int(b) == 1, k
        else:
            bufs.append((k, rel_l2(b, P[k].detach())))
    wg, wb = max(grads, key=lambda kv: kv[1]), max(bufs, key=lambda kv: kv[1])
    print(f"two-rank step {case} {shape}: logits {e_logits:.2e}, loss {e_loss:.2e}, worst gradient {wg[0]} {wg[1]:.2e}, "
          f"worst running buffer {wb[0]} {wb[1]:.2e}")
    # beside it: the single-rank HIP step on the full batch against the same oracle quantities that do not depend on the sharding (logits,
    # running buffers; its loss and gradients belong to the full-batch pos_weight, a different objective)
    net1 = _seeded_net(7).to(cuda).train()
    l1, _ = _hip_step(net1, x, labels, cuda)
    torch.cuda.synchronize()
    b1 = max(rel_l2(b.cpu(), P[k].detach()) for k, b in net1.named_buffers() if not k.endswith("num_batches_tracked"))
    print(f"  single-rank HIP step on the full batch: logits {rel_l2(l1.cpu(), lref):.2e}, worst running buffer {b1:.2e}")
    assert len(grads) == len(list(net1.parameters()))
    assert e_logits <= NET_TOL and e_loss <= NET_TOL, (e_logits, e_loss)
    bad = [(k, e) for k, e in grads + bufs if not e <= NET_TOL]
    assert not bad, bad


# 3. running statistics: the same bits on every rank
@pytest.mark.timeout(900)
@pytest.mark.parametrize("case", list(_STEP_CASES))
def test_running_buffers_bit_equal_on_all_ranks(cuda, case, tmp_path_factory):
    ranks = _two_rank_step(case, tmp_path_factory)
    a, b = ranks[0]["buffers"], ranks[1]["buffers"]
    assert a.keys() == b.keys() and len(a) == 3 * 37
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, f"running buffers differ between the ranks: {diff[:5]}"
    assert all(int(v) == 1 for k, v in a.items() if k.endswith("num_batches_tracked"))
    assert ranks[0]["grad_digest"] == ranks[1]["grad_digest"], "averaged gradients differ between the ranks"


# 4. determinism: no atomics, fixed merge order, gathered (not all-reduced) partial sums
@pytest.mark.timeout(900)
def test_two_rank_step_is_bit_reproducible(cuda, tmp_path_factory):
    for r in _two_rank_step("2+2", tmp_path_factory):
        assert not r["grads_differ_second_run"], f"gradients differ between two identical two-rank steps: {r['grads_differ_second_run'][:5]}"
        assert r["grad_digest"] == r["grad_digest_second_run"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. three data-parallel AdamW steps on two ranks, then eval()
# ---------------------------------------------------------------------------------------------------------------------------------
def _train_worker(rank: int, world: int, port: int, q):
    _init(rank, world, port)
    try:
        from oracle import onsetnet_ref
        from syncfusion_amd import OnsetModel, allreduce_gradients

        cuda = torch.device("cuda:0")
        net = _seeded_net(7)
        model = nn.SyncBatchNorm.convert_sync_batchnorm(OnsetModel(1e-3, 0.9, 0.999, 1e-8, 1e-2, net)).to(cuda)
        net = model.model
        opt = model.configure_optimizers()
        xe = torch.randn(2, 3, 4, 32, 32, generator=torch.Generator().manual_seed(8))
        with torch.no_grad():
            before = net.eval()(xe.to(cuda)).cpu()     # the inference engine of a converted net, on the initial weights
        net.train()
        x, labels = _data((4, 3, 4, 32, 32), 21, 22)
        lo, hi = _spans((3, 1))[rank]
        batch = {"frames": x[lo:hi].to(cuda), "label": labels[lo:hi].to(cuda)}
        for i in range(3):
            opt.zero_grad(set_to_none=True)
            loss = model.training_step(batch, i)
            loss.backward()
            allreduce_gradients(model)
            opt.step()
        with torch.no_grad():
            y = net.eval()(xe.to(cuda)).cpu()
            ref = onsetnet_ref.onsetnet_forward({k: v.detach().float().cpu() for k, v in net.state_dict().items()}, xe)
        q.put((rank, {"err": rel_l2(y, ref), "moved": rel_l2(before, ref), "nbt": int(net.net.model.stem[1].num_batches_tracked),
                      "state_digest": _digest(net.state_dict().values())}))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_eval_engine_follows_data_parallel_training(cuda):
    res = _spawn(_train_worker, 2, (), 600)
    for rank in range(2):
        r = res[rank]
        print(f"rank {rank}: eval engine after 3 data-parallel AdamW steps: rel-L2 {r['err']:.2e} (moved {r['moved']:.2e} from the initial logits)")
        assert r["nbt"] == 3
        assert r["moved"] > 10 * NET_TOL, "the steps did not change the logits"
        assert r["err"] < NET_TOL
    assert res[0]["state_digest"] == res[1]["state_digest"], "parameters / buffers differ between the ranks after three steps"


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. routing
# ---------------------------------------------------------------------------------------------------------------------------------
def _plain_and_converted(cuda):
    x, labels = _data((2, 3, 4, 32, 32), 2, 5)
    plain = _seeded_net(7).to(cuda).train()
    conv = nn.SyncBatchNorm.convert_sync_batchnorm(_seeded_net(7)).to(cuda).train()
    assert sum(isinstance(m, nn.SyncBatchNorm) for m in conv.modules()) == 37
    return x, labels, plain, conv


def _assert_same_step(plain, conv, x, labels, cuda, what):
    l0, loss0 = _hip_step(plain, x, labels, cuda)
    l1, loss1 = _hip_step(conv, x, labels, cuda)
    torch.cuda.synchronize()
    assert torch.equal(l0, l1) and torch.equal(loss0, loss1), f"{what}: logits differ from the unconverted net"
    g0, g1 = dict(plain.named_parameters()), dict(conv.named_parameters())
    assert g0.keys() == g1.keys()
    diff = [k for k in g0 if not torch.equal(g0[k].grad, g1[k].grad)]
    assert not diff, f"{what}: gradients differ from the unconverted net: {diff[:5]}"
    b0, b1 = dict(plain.named_buffers()), dict(conv.named_buffers())
    assert not [k for k in b0 if not torch.equal(b0[k], b1[k])]


def test_converted_net_without_process_group_runs_the_plain_path(cuda):
    assert not dist.is_initialized()
    x, labels, plain, conv = _plain_and_converted(cuda)
    _assert_same_step(plain, conv, x, labels, cuda, "no process group")
    # eval(): the inference engine of the converted net, bit-equal to the unconverted engine
    with torch.no_grad():
        assert torch.equal(plain.eval()(x.to(cuda)), conv.eval()(x.to(cuda)))


@pytest.mark.timeout(600)
def test_converted_net_in_a_world_of_one_runs_the_plain_path(cuda):
    assert not dist.is_initialized()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        x, labels, plain, conv = _plain_and_converted(cuda)
        _assert_same_step(plain, conv, x, labels, cuda, "world size 1")
    finally:
        dist.destroy_process_group()


def _zero_clip_worker(rank: int, world: int, port: int, q):
    _init(rank, world, port)
    try:
        cuda = torch.device("cuda:0")
        net = nn.SyncBatchNorm.convert_sync_batchnorm(_seeded_net(7)).to(cuda).train()
        x, _ = _data((2, 3, 4, 32, 32))
        mine = x if rank == 0 else x[:0]          # rank 1 holds no clips
        try:
            net(mine.to(cuda))
            msg = None
        except ValueError as e:
            msg = str(e)
        q.put((rank, msg))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_rank_with_zero_clips_raises(cuda):
    res = _spawn(_zero_clip_worker, 2, (), 400)
    for rank in range(2):     # every rank sees the gathered clip counts and raises: nobody is left waiting in a collective
        assert res[rank] is not None and "no clips" in res[rank] and "[1]" in res[rank], res[rank]


def test_capture_of_a_synchronised_step_is_refused(cuda, monkeypatch):
    """HIP-graph capture of a synchronised step is out of scope: the op raises before it launches anything.  (The capture state is
    reported through torch.cuda.is_current_stream_capturing; the test answers for it instead of opening a real capture.)"""
    from syncfusion_amd.onset_training import SyncGroup, batch_norm_train_sync

    bn = nn.BatchNorm3d(8).to(cuda)
    x = torch.randn(64, 8, device=cuda, requires_grad=True)
    sg = SyncGroup(None, 1, cuda)
    y = batch_norm_train_sync(x, bn, sg)
    assert int(bn.num_batches_tracked) == 1
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        batch_norm_train_sync(x, bn, sg)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        y.sum().backward()
    assert int(bn.num_batches_tracked) == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the nccl (RCCL) path with one rank: device tensors straight into the collectives
# ---------------------------------------------------------------------------------------------------------------------------------
def _rccl_worker(rank: int, world: int, port: int, q):
    _init(rank, world, port, backend="nccl")
    try:
        from syncfusion_amd.module_onset import BCLoss
        from syncfusion_amd.onset_training import onset_train_forward

        cuda = torch.device("cuda:0")
        torch.cuda.set_device(cuda)
        x, labels = _data((2, 3, 4, 32, 32), 2, 5)
        plain = _seeded_net(7).to(cuda).train()
        lp, _ = _hip_step(plain, x, labels, cuda)
        calls = {"n": 0, "on_device": True}
        real = dist.all_gather_into_tensor

        def counted(out, inp, *a, **k):
            calls["n"] += 1
            calls["on_device"] &= bool(out.is_cuda and inp.is_cuda)
            return real(out, inp, *a, **k)

        dist.all_gather_into_tensor = counted
        split = nn.SyncBatchNorm.convert_sync_batchnorm(_seeded_net(7)).to(cuda).train()
        logits = onset_train_forward(split, x.to(cuda), _force_sync=True)
        loss = BCLoss()(logits, labels.to(cuda))
        loss.backward()
        torch.cuda.synchronize()
        dist.all_gather_into_tensor = real
        g0, g1 = dict(plain.named_parameters()), dict(split.named_parameters())
        b0, b1 = dict(plain.named_buffers()), dict(split.named_buffers())
        out = {"backend": dist.get_backend(), "gathers": calls["n"], "on_device": calls["on_device"],
               "logits": rel_l2(logits.detach().cpu(), lp.cpu()),
               "grad": max(rel_l2(g1[k].grad.cpu(), g0[k].grad.cpu()) for k in g0),
               "buffer": max(rel_l2(b1[k].cpu(), b0[k].cpu()) for k in b0 if not k.endswith("num_batches_tracked")),
               "nbt": int(split.net.model.stem[1].num_batches_tracked)}
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_split_phase_step_over_rccl_with_one_rank(cuda):
    r = _spawn(_rccl_worker, 1, (), 600)[0]
    print(f"split-phase step over RCCL, one rank, against the plain path: logits {r['logits']:.2e}, worst gradient {r['grad']:.2e}, "
          f"worst running buffer {r['buffer']:.2e}; {r['gathers']} device all-gathers")
    assert r["backend"] == "nccl" and r["on_device"]
    assert r["gathers"] == 2 * 37, r["gathers"]     # one per BatchNorm and direction (the clip counts ride in their own gather)
    assert r["nbt"] == 1
    assert r["logits"] <= TOL and r["grad"] <= TOL and r["buffer"] <= TOL, r
