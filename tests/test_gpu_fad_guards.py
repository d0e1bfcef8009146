"""Guard-band tests (MI355X) of the FAD entry points: the front end, the max-pool at odd extents, the VGGish forward and the moments write
and read nothing outside the buffers they are handed (tests/guards.py).  Every device pointer argument sits inside guard bands; the
workspace has exactly the size the query reports; outputs are compared bit for bit with a run on ordinary allocations."""
import ctypes as C

import pytest
import torch

import fad_ref
from guards import Guards

pytestmark = pytest.mark.gpu


def narrow_model(device):
    from syncfusion_amd.fad import VGGish, VGGishConfig

    m = VGGish(VGGishConfig(layout=fad_ref.NARROW_LAYOUT, fc=fad_ref.NARROW_FC))
    m.load_state_dict(fad_ref.seeded_weights(fad_ref.NARROW_LAYOUT, fad_ref.NARROW_FC, 11))
    return m.to(device)


def check(rc, what):
    from syncfusion_amd import _lib

    assert rc == 0, f"{what}: code {rc}: {_lib.load().sf_last_error()}"


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_front_end_guarded(cuda):
    from syncfusion_amd import _lib

    model = narrow_model(cuda)
    wav = fad_ref.clip_signal(1, 15600, 3).to(cuda)
    plain_rows, plain_mel = model._front_call(wav, True)
    with Guards(cuda) as g:
        x = g.inp(wav, "wav")
        rows = g.out((96 * 64, 4), name="examples")
        mel = g.out((1, 96, 64), name="mel")
        with torch.cuda.device(cuda):
            check(_lib.load().sf_logmel_examples_forward(model._front_end(), x.ptr, 1, 15600, 96, 0.01, rows.ptr, mel.ptr, _lib.stream_ptr(cuda)),
                  "sf_logmel_examples_forward")
    assert bool(torch.isfinite(rows.payload).all()) and same_bits(rows.payload, plain_rows) and same_bits(mel.payload, plain_mel)


@pytest.mark.parametrize("ld", [8, 3])          # the 4-column vector kernel and the element kernel
def test_maxpool_odd_extents_guarded(cuda, ld):
    from syncfusion_amd import _lib

    n, H, W = 2, 3, 5
    g0 = torch.Generator().manual_seed(ld)
    x = torch.randn(n, H, W, ld, generator=g0)
    ref = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()      # floor: (2, 1, 2, ld)
    with Guards(cuda) as g:
        xi = g.inp(x.to(cuda), "x")
        y = g.out((n, H // 2, W // 2, ld), name="y")
        with torch.cuda.device(cuda):
            check(_lib.load().sf_op_maxpool2x2_cl(xi.ptr, n, H, W, ld, y.ptr, _lib.stream_ptr(cuda)), "sf_op_maxpool2x2_cl")
    assert torch.equal(y.payload.cpu(), ref)


def test_vggish_forward_guarded(cuda):
    from syncfusion_amd import _lib

    lib = _lib.load()
    model = narrow_model(cuda)
    ex, _ = fad_ref.examples(fad_ref.clip_signal(1, 15600, 3).double().numpy())
    rows = torch.zeros((96 * 64, 4))
    rows[:, 0] = torch.from_numpy(ex).float().reshape(-1)
    rows = rows.to(cuda)
    plain, plain_pools = model.embed_rows(rows, pool_taps=True)
    eng = model._engine_for(cuda)
    shapes = [(1, 48, 32, 8), (1, 24, 16, 16), (1, 12, 8, 24), (1, 6, 4, 40)]          # padded channel counts of 8, 12, 20, 36
    with Guards(cuda) as g:
        x = g.inp(rows, "examples")
        emb = g.out((1, 24), name="embeddings")
        taps = [g.out(s, name=f"pool{i}") for i, s in enumerate(shapes)]
        ws = g.ws(int(lib.sf_vggish_workspace_bytes(eng, 1)), "workspace")
        arr = (C.c_void_p * 4)(*[t.ptr for t in taps])
        with torch.cuda.device(cuda):
            check(lib.sf_vggish_forward(eng, x.ptr, 1, emb.ptr, arr, ws.ptr, ws.nbytes, _lib.stream_ptr(cuda)), "sf_vggish_forward")
    assert bool(torch.isfinite(emb.payload).all()) and same_bits(emb.payload, plain)
    for t, p, s in zip(taps, plain_pools, shapes):
        assert same_bits(t.payload[..., :p.shape[-1]], p)
        assert bool((t.payload[..., p.shape[-1]:] == 0).all()), "padding columns stay zero through the pools"


def test_moments_guarded(cuda):
    from syncfusion_amd import _lib
    from syncfusion_amd.fad import embedding_moments

    g0 = torch.Generator().manual_seed(9)
    x = torch.randn(97, 24, generator=g0).to(cuda)
    plain = embedding_moments(x)
    with Guards(cuda) as g:
        xi = g.inp(x, "embeddings")
        s = g.out((24,), torch.float64, name="sum")
        sc = g.out((24, 24), torch.float64, name="scatter")
        with torch.cuda.device(cuda):
            check(_lib.load().sf_op_moments(xi.ptr, 97, 24, s.ptr, sc.ptr, _lib.stream_ptr(cuda)), "sf_op_moments")
    assert same_bits(s.payload.cpu(), torch.from_numpy(plain.sum)) and same_bits(sc.payload.cpu(), torch.from_numpy(plain.scatter))
