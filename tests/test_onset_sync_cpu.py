"""CPU suite for the onset net's cross-rank BatchNorm (syncfusion_amd/onset_training.py, sf_op_bn_sync_*): the split-phase symbols are
declared in the header and bound in _lib.py, the module surface (convert_sync_batchnorm keeps the state_dict keys), and -- over a gloo world
of 2 on CPU tensors -- which modules take the synchronised path, the clip-count gather, the row-count table and the rank-order all-gather.
No kernel runs here."""
import os
import re
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from helpers import ROOT

SYNC_SYMBOLS = ("sf_op_bn_sync_workspace_bytes", "sf_op_bn_sync_stats", "sf_op_bn_sync_fwd_apply", "sf_op_bn_sync_bwd_sums",
                "sf_op_bn_sync_bwd_apply")


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _collect(procs, q, seconds: float):
    """One result per worker; a worker that died (non-zero exit) fails the test at once instead of after the queue's timeout."""
    import queue
    import time

    out, deadline = [], time.monotonic() + seconds
    try:
        while len(out) < len(procs):
            try:
                out.append(q.get(timeout=1.0))
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


def test_sync_symbols_declared_bound_and_exported():
    from syncfusion_amd import _lib

    header = open(os.path.join(ROOT, "include", "syncfusion_amd.h")).read()
    declared = set(re.findall(r"\b(sf_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in SYNC_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/syncfusion_amd.h"
        assert name in _lib.SYMBOLS, f"{name} is not bound in _lib.py"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    # the workspace query is a host-only call: rows >= 1 (a rank may hold a single row), the same size formula as the plain op at rows >= 2
    assert lib.sf_op_bn_sync_workspace_bytes(0, 8) == -1 and lib.sf_op_bn_sync_workspace_bytes(4, 0) == -1
    assert lib.sf_op_bn_sync_workspace_bytes(1, 45) >= (2 * 45 + 3 * 45) * 4
    for rows, Cc in ((2, 45), (4096, 64), (6021120, 512)):
        assert lib.sf_op_bn_sync_workspace_bytes(rows, Cc) == lib.sf_op_bn_train_workspace_bytes(rows, Cc)


def test_split_phase_calls_check_their_arguments():
    """Null pointers, a bad row length and a short workspace are refused before anything is launched (host-only: no device is touched)."""
    from syncfusion_amd import _lib

    lib = _lib.load()
    assert lib.sf_op_bn_sync_stats(None, 4, 8, 8, None, None, 0, None) != 0
    assert b"null" in lib.sf_last_error()
    buf = torch.zeros(64)
    p = buf.data_ptr()
    assert lib.sf_op_bn_sync_stats(p, 4, 8, 6, p, p, 1 << 20, None) != 0          # ld % 4
    assert lib.sf_op_bn_sync_stats(p, 4, 8, 8, p, p, 8, None) != 0                # workspace too small
    assert b"workspace" in lib.sf_last_error()
    assert lib.sf_op_bn_sync_fwd_apply(p, None, 4, 8, 8, p, p, 0, p, p, 1e-5, 0.1, None, None, None, 0, p, p, p, p, 1 << 20, None) != 0   # world 0
    assert lib.sf_op_bn_sync_bwd_apply(p, None, p, 4, 8, 8, p, p, 2, p, p, p, None, None, p, 1 << 20, None) != 0          # nothing to compute


def test_convert_sync_batchnorm_keeps_the_checkpoint_keys():
    from syncfusion_amd import OnsetModel, VideoOnsetNet, allreduce_gradients  # noqa: F401  (the export OnsetModel users look for)

    net = VideoOnsetNet(False)
    keys = list(net.state_dict().keys())
    conv = nn.SyncBatchNorm.convert_sync_batchnorm(net)
    assert conv is net and list(conv.state_dict().keys()) == keys
    bns = [m for m in conv.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
    assert len(bns) == 37 and all(isinstance(m, nn.SyncBatchNorm) for m in bns)
    model = nn.SyncBatchNorm.convert_sync_batchnorm(OnsetModel(1e-4, 0.9, 0.999, 1e-8, 1e-2, VideoOnsetNet(False)))
    assert sum(isinstance(m, nn.SyncBatchNorm) for m in model.modules()) == 37


def test_no_process_group_selects_the_plain_path():
    from syncfusion_amd.onset_training import _SyncState

    assert not dist.is_initialized()
    st = _SyncState(2, torch.device("cpu"))
    assert st.group_for(nn.SyncBatchNorm(4)) is None and st.group_for(nn.BatchNorm3d(4)) is None
    # forced (tests, tools): a world of one whose gather is a reshape
    sg = _SyncState(2, torch.device("cpu"), force=True).group_for(nn.BatchNorm3d(4))
    assert sg is not None and sg.world == 1 and sg.clips == [2] and sg.collectives == 0
    local = torch.arange(8.0).view(4, 2)
    assert torch.equal(sg.all_gather(local), local.view(1, 4, 2))
    assert sg.row_counts(7).tolist() == [14] and sg.row_counts(7).dtype == torch.int64


def _worker(rank: int, world: int, port: int, clips, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from syncfusion_amd.onset_training import _SyncState

        cpu = torch.device("cpu")
        out = {}
        st = _SyncState(clips[rank], cpu)
        sbn, sbn2, bn = nn.SyncBatchNorm(4), nn.SyncBatchNorm(6), nn.BatchNorm3d(4)
        out["plain_module"] = st.group_for(bn) is None
        sg = st.group_for(sbn)
        out["same_group_once"] = st.group_for(sbn2) is sg and sg.collectives == 1      # one clip-count gather per forward
        out["clips"], out["rank"], out["world"] = sg.clips, sg.rank, sg.world
        rc = sg.row_counts(5 * 3 * 3)
        out["row_counts"] = (rc.tolist(), str(rc.dtype), sg.row_counts(45) is rc, sg.total_rows(45))
        local = torch.full((4, 2), float(10 * rank)) + torch.arange(8.0).view(4, 2)
        out["table"] = sg.all_gather(local).tolist()
        out["collectives"] = sg.collectives
        # a group of one rank (this rank alone) -> the plain path, as torch.nn.SyncBatchNorm itself
        solo = [dist.new_group([r]) for r in range(world)][rank]
        one = nn.SyncBatchNorm(4, process_group=solo)
        out["world1_group_plain"] = _SyncState(clips[rank], cpu).group_for(one) is None
        # a rank without clips: every rank sees the gathered table and raises, nobody waits in a collective
        try:
            _SyncState(0 if rank == 1 else 2, cpu).group_for(sbn)
            out["zero_raises"] = None
        except ValueError as e:
            out["zero_raises"] = str(e)
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_path_selection_and_clip_gather_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    clips = (3, 1)
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, clips, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(_collect(procs, q, 240))
    want_table = [(torch.full((4, 2), float(10 * r)) + torch.arange(8.0).view(4, 2)).tolist() for r in range(2)]
    for rank in range(2):
        o = res[rank]
        assert o["plain_module"] and o["same_group_once"] and o["world1_group_plain"]
        assert o["clips"] == [3, 1] and o["rank"] == rank and o["world"] == 2
        assert o["row_counts"] == ([135, 45], "torch.int64", True, 180)
        assert o["table"] == want_table, "the gathered table is not in rank order"
        assert o["collectives"] == 2
        assert o["zero_raises"] is not None and "rank(s) [1]" in o["zero_raises"] and "no clips" in o["zero_raises"]
