"""Guard-band test (tests/guards.py) of ``sf_op_onset_test_step``: logits and labels as inputs, the four epoch tables and the sums as
in-place buffers, the workspace at EXACTLY ``sf_op_onset_test_workspace_bytes(N, T)``, every one inside guard bands; rows
[clip0, clip0 + N) with clip0 > 0 of tables whose capacity lies above clip0 + N.  Asserted: return code 0, every guard untouched, the
inputs unchanged, and every table and the sums byte-equal to a run on ordinary allocations (rows outside the batch included: they keep
their initial values).  (1, 1) is a one-class batch: its AP / Acc sums are NaN in both runs, with equal bits."""
import pytest
import torch

from guards import Guards

pytestmark = pytest.mark.gpu

CLIP0, SPARE = 2, 3          # rows in front of the batch, rows behind it


class _Plain:
    """Ordinary allocations behind the part of the ``Guards`` interface used here."""

    class _T:
        def __init__(self, t):
            self.payload, self.ptr = t, t.data_ptr()

    def __init__(self, device):
        self.device = device

    def inp(self, t, name=""):
        return self._T(t.to(self.device).contiguous().clone())

    inout = inp

    def ws(self, nbytes, name=""):
        return self._T(torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=self.device))

    def verify_all(self):
        torch.cuda.synchronize(self.device)


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


@pytest.mark.parametrize("N,T", [(1, 1), (3, 30), (4, 65)])
def test_onset_test_step_stays_inside_its_buffers(cuda, N, T):
    from syncfusion_amd import _lib

    lib = _lib.load()
    g = torch.Generator().manual_seed(10 * N + T)
    z = (torch.randint(-512, 513, (N, T), generator=g) / 64.0).to(cuda)
    t = (torch.rand(N, T, generator=g) < 0.3).float()
    t[0, 0] = 1.0
    if T > 1:
        t[0, 1] = 0.0
    t = t.to(cuda)
    cap = CLIP0 + N + SPARE
    counts0 = torch.arange(100, 100 + cap, dtype=torch.int32, device=cuda)
    frames0 = torch.arange(1000, 1000 + cap * T, dtype=torch.int32, device=cuda).view(cap, T)
    sums0 = torch.tensor([1.5, 2.5, 0.25, 0.5, 3.0], dtype=torch.float64, device=cuda)
    nws = int(lib.sf_op_onset_test_workspace_bytes(N, T))
    assert nws > 0

    def run(a):
        zs, ts = a.inp(z, "logits"), a.inp(t, "labels")
        tabs = [a.inout(counts0, "pred_count"), a.inout(frames0, "pred_frames"), a.inout(counts0, "target_count"), a.inout(frames0, "target_frames")]
        sums = a.inout(sums0, "sums")
        wk = a.ws(nws, "ws")
        rc = lib.sf_op_onset_test_step(zs.ptr, ts.ptr, N, T, 0.5, 0.75, CLIP0, cap, *[x.ptr for x in tabs], sums.ptr, wk.ptr, nws, _lib.stream_ptr(cuda))
        assert rc == 0, lib.sf_last_error().decode()
        a.verify_all()
        return tabs + [sums]

    plain = run(_Plain(cuda))
    guarded = run(Guards(cuda))
    for p, q in zip(plain, guarded):
        assert torch.equal(_bytes(p.payload), _bytes(q.payload)), q.name
    pc, pf, tc, tf, sums = (x.payload for x in guarded)
    for tab, init in ((pc, counts0), (pf, frames0), (tc, counts0), (tf, frames0)):
        assert torch.equal(tab[:CLIP0], init[:CLIP0]) and torch.equal(tab[CLIP0 + N:], init[CLIP0 + N:])       # rows outside the batch
    want_pred = (z > 0.5).sum(dim=1).to(torch.int32)
    assert torch.equal(pc[CLIP0: CLIP0 + N], want_pred) and torch.equal(tc[CLIP0: CLIP0 + N], (t != 0).sum(dim=1).to(torch.int32))
    assert float(sums[4]) == 3.0 + N
    if N * T == 1:
        assert bool(torch.isnan(sums[1:3]).all()) and bool(torch.isfinite(sums[3]))
    else:
        assert bool(torch.isfinite(sums).all())
