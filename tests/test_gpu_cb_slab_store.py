"""conv_cb's partial-slab stores (MI355X): the fp32 slabs leave the kernel as 16-byte buffer stores, a wave's 32 x 32 tile passed through
LDS so that one store instruction writes 8 whole 128-byte rows (8 lanes x 16 B) of the workgroup's own slab, rows past M dropped by the
buffer resource.  The shapes are the smallest at which that lane -> (row, column quad) mapping can go wrong:

  (3, 44, 256, 1)    S = 2 slabs, one-tile workgroups, M = 132: the last tile has 4 live rows
  (3, 44, 256, 2)    the same with two channel blocks per workgroup (one slab)
  (3, 44, 1024, 1)   S = 8; 3 x 64 = 192 workgroups >= 160, so two row tiles per workgroup; the last 64-row workgroup has 4 live rows
  (2, 50, 1024, 1)   M = 100, one tile per workgroup, clips ending inside a tile

each in bf16 and fp16 through sf_op_resnet_mod_cb (both convolutions of the chain: without and with the GroupNorm panel prologue).
  (a) h and m against torch in fp64 from the same 16-bit-rounded inputs, at test_gpu_ops.test_conv_cb_chain's tolerance;
  (b) the op run twice with the whole workspace (slabs included) pre-filled with two different poison patterns, quiet NaNs and 1e30:
      h and m are bit-equal between the runs and finite, so every slab element the reducers read was written by this call -- no row and
      no column quad was skipped, whatever the stores' layout.
"""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_ops import TD, TOL

pytestmark = pytest.mark.gpu

SHAPES = [(3, 44, 256, 1), (3, 44, 256, 2), (3, 44, 1024, 1), (2, 50, 1024, 1)]   # B, L, C, channel blocks per workgroup


def _lib():
    from syncfusion_amd import _lib

    return _lib, _lib.load()


def _rel(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_slab_stores_cover_every_element(cuda, dtype, shape):
    _l, lib = _lib()
    B, L, C, kb = shape
    G = 8
    td = TD[dtype]
    g = torch.Generator().manual_seed(B * 1000 + L + C + kb)
    x = torch.randn(B, C, L, generator=g) * 1.3 + 0.2
    w1 = torch.randn(C, C, 3, generator=g) / (3 * C) ** 0.5
    w2 = torch.randn(C, C, 3, generator=g) / (3 * C) ** 0.5
    b1, b2 = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    gam = [1 + 0.2 * torch.randn(C, generator=g) for _ in range(2)]
    bet = [0.1 * torch.randn(C, generator=g) for _ in range(2)]
    ss = torch.randn(B, 2 * C, generator=g) * 0.3
    d = lambda t: t.double()   # noqa: E731
    xr = x.to(td).double()
    h_ref = F.conv1d(F.silu(F.group_norm(xr, G, d(gam[0]), d(bet[0]), eps=1e-5)), w1.to(td).double(), d(b1), padding=1)
    y = xr + F.conv1d(F.silu(F.group_norm(h_ref, G, d(gam[1]), d(bet[1]), eps=1e-5)), w2.to(td).double(), d(b2), padding=1)
    m_ref = F.layer_norm(y.transpose(1, 2), (C,), eps=1e-6) * (1 + d(ss)[:, None, :C]) + d(ss)[:, None, C:]
    dev = lambda t: t.to(cuda)   # noqa: E731
    x_cl = dev(x.transpose(1, 2).contiguous().to(td))
    keep = [dev(t) for t in (w1, b1, w2, b2, gam[0], bet[0], gam[1], bet[1])]
    ssd = dev(ss)
    nbytes = int(lib.sf_op_resnet_mod_cb_workspace_bytes(B, L, C))
    assert nbytes > 0 and nbytes % 4 == 0
    runs = []
    for poison in (torch.tensor(0x7FC00000, dtype=torch.int32).view(torch.float32).item(), 1e30):
        ws = torch.full((nbytes // 4,), poison, dtype=torch.float32, device=cuda)
        h = torch.full((B, L, C), float("nan"), dtype=td, device=cuda)
        m = torch.full((B, L, C), float("nan"), dtype=td, device=cuda)
        _l.check(lib.sf_op_resnet_mod_cb(_l.DTYPES[dtype], x_cl.data_ptr(), *[t.data_ptr() for t in keep], G, 1e-5, ssd.data_ptr(), 1e-6,
                                         B, L, C, kb, h.data_ptr(), m.data_ptr(), ws.data_ptr(), nbytes, _l.stream_ptr(cuda)), "sf_op_resnet_mod_cb")
        torch.cuda.synchronize()
        runs.append((h.cpu(), m.cpu()))
    (h0, m0), (h1, m1) = runs
    e_h, e_m = _rel(h0.transpose(1, 2), h_ref), _rel(m0, m_ref)
    print(f"conv_cb slab stores {dtype} {shape}: h {e_h:.3e}  m {e_m:.3e}")
    assert e_h < TOL[dtype] and e_m < TOL[dtype]
    i16 = torch.int16
    assert torch.isfinite(h0.float()).all() and torch.isfinite(m0.float()).all()
    assert torch.equal(h0.view(i16), h1.view(i16)) and torch.equal(m0.view(i16), m1.view(i16))
