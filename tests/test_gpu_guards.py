"""Guard-band tests (MI355X): no C-ABI entry writes or reads outside the buffers it is handed.

Every case builds seeded inputs as the op tests do, runs the entry once on ordinary allocations (the plain run) and once with EVERY
device pointer argument -- inputs, outputs, optional outputs, workspaces, pack buffers, stats and lse buffers -- inside guard bands
(tests/guards.py), then asserts: return code 0, every guard untouched and every input payload unchanged (verify_all), every guarded
output finite, every guarded output equal to the plain run.  Workspaces get EXACTLY the size the matching query reports
(sf_*_workspace_bytes, sf_op_gn_silu_train_stats_floats, sf_op_conv1d_dgrad_pack_bytes); sf_op_conv1d_cl / sf_op_conv1d_train_fwd have
no query and get syncfusion_amd.autograd.conv1d_workspace_bytes (the production caller's size), sf_op_gn_silu gets the
B * 32 * groups * 2 floats its header comment states, and the attention backward gets the smallest size capi_train.cpp accepts
(B * heads * L * 4 bytes: `need` in attention_bwd_lse_impl).

Outputs are compared with the plain run bit for bit (byte equality, which also holds NaN by contract to equal bits).  Entries compared
by tolerance instead: none.  The header promises identical bits for the training, loss, optimizer and augment entries; the inference
entries run the same launches on the same inputs in both runs and are held to the same standard.

Engines (sf_unet_forward, sf_vsample, sf_encoder1d_forward, sf_onsetnet_forward): the plain run goes through the Python engine object;
the guarded run calls the same entry on the same handle, because the wrappers allocate their outputs themselves and an output can only
be guarded from outside.  The workspace is exactly the engine's *_workspace_bytes.  These cases see the two ENDS of the workspace
only, not the boundaries between the sub-buffers the engine carves out of it.

Limits:
  * a read past an input whose value is masked out by a select (not by arithmetic) is not detected;
  * writes further away than one guard (max(64 KiB, 256 rows)) are not detected;
  * nothing here inspects code objects or assembly; which kernel family a shape reaches is the dispatcher's decision (DESIGN.md
    section 4), the comments name the family each shape was chosen for.
"""
import ctypes as ct

import pytest
import torch

from guards import Guards
from helpers import SMALL_ENCODER, SMALL_UNET, seeded_state, small_encoder_module, small_unet_module, synth_inputs

pytestmark = pytest.mark.gpu

TD = {"fp32": torch.float32, "fp32x": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
REPEAT_PLAIN = False      # measurement aid: run the plain call twice and record run-to-run bit equality per entry
REPEAT_LOG = []


def _lib():
    from syncfusion_amd import _lib

    return _lib, _lib.load()


class _PlainT:
    def __init__(self, t):
        self.payload, self.ptr = t, t.data_ptr()


class Plain:
    """The allocator of the plain run: ordinary torch allocations behind the interface of guards.Guards."""

    def __init__(self, device):
        self.device, self.outs = device, []

    def inp(self, t, name="", ld=None):
        return _PlainT(t.to(self.device).contiguous().clone())

    inout = inp

    def out(self, shape, dtype=torch.float32, name="", ld=None):
        t = torch.empty(shape, dtype=dtype, device=self.device)
        t.view(-1).view(torch.uint8).fill_(0xFF)
        self.outs.append(t)
        return _PlainT(t)

    def ws(self, nbytes, name="", ld=None):
        t = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.device)
        t.fill_(0xFF)
        return _PlainT(t)


class _G(Guards):
    """guards.Guards that moves inputs to the device first (the cases hand in CPU or device tensors)."""

    def inp(self, t, name="", ld=None):
        return super().inp(t.to(self.device).contiguous(), name, ld)

    def inout(self, t, name="", ld=None):
        return super().inout(t.to(self.device).contiguous(), name, ld)


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _run_case(cuda, entry, run, nan_ok=()):
    """run(a) -> (rc, [compared tensors' holders]); a is Plain or Guards.  nan_ok: indices of compared tensors whose contract allows NaN."""
    plain = Plain(cuda)
    rc, pouts = run(plain)
    assert rc == 0, f"{entry} (plain): rc {rc}: {_lib()[1].sf_last_error().decode()}"
    torch.cuda.synchronize()
    if REPEAT_PLAIN:
        rc2, pouts2 = run(Plain(cuda))
        torch.cuda.synchronize()
        REPEAT_LOG.append((entry, rc2 == 0 and all(torch.equal(_bytes(a.payload), _bytes(b.payload)) for a, b in zip(pouts, pouts2))))
    g = _G(cuda)
    rc, gouts = run(g)
    assert rc == 0, f"{entry} (guarded): rc {rc}: {_lib()[1].sf_last_error().decode()}"
    g.verify_all()
    assert len(pouts) == len(gouts) and len(gouts) > 0
    for i, (p, q) in enumerate(zip(pouts, gouts)):
        if q.payload.is_floating_point() and i not in nan_ok:
            bad = ~torch.isfinite(q.payload)
            assert not bool(bad.any()), f"{entry}: {q.name}: {int(bad.sum())} non-finite values, first at flat index {int(bad.flatten().nonzero()[0])}"
        same = torch.equal(_bytes(p.payload), _bytes(q.payload))
        if not same:
            d = (_bytes(p.payload) != _bytes(q.payload)).nonzero().flatten()
            raise AssertionError(f"{entry}: {q.name} differs from the plain run in {d.numel()} bytes, offsets {int(d[0])} .. {int(d[-1])}")


def _ptr(h):
    return h.ptr if h is not None else None


# ---------------------------------------------------------------------------------------------------------------------------------
# sf_op_conv1d_cl
# ---------------------------------------------------------------------------------------------------------------------------------
CONV_SHAPES = [
    # B, L, C, N, taps, stride, pad, up, groups, residual
    (5, 3, 64, 64, 3, 1, 1, 1, 8, False),          # clips shorter than the halo
    (1, 1000, 64, 96, 3, 1, 1, 1, 4, False),       # ragged M and N
    (2, 100, 256, 320, 1, 1, 0, 1, 0, False),      # ragged on the 32x32 families
    (9, 5000, 128, 320, 1, 1, 0, 1, 0, False),     # macro tiles with ragged M and a partial column tile
    (3, 3000, 256, 192, 1, 1, 0, 1, 0, False),     # fp32 macro tiles
    (4, 88, 1024, 1024, 3, 1, 1, 1, 0, True),      # wave-private split-K
    (5, 61, 256, 256, 3, 1, 1, 1, 0, True),        # register-staged tap bookkeeping
    (8, 44, 512, 256, 3, 1, 1, 1, 0, True),        # clips shorter than a tile
    (2, 88, 64, 8, 3, 1, 1, 4, 0, False),          # x4 upsample with N < 32
    (2, 352, 32, 64, 5, 2, 2, 1, 0, False),        # strided
    (3, 500, 16, 32, 9, 4, 4, 1, 0, False),        # thin / direct shapes
    (2, 704, 1, 8, 1, 1, 0, 1, 0, False),
    (2, 704, 8, 1, 3, 1, 1, 1, 0, True),
    (2, 640, 2, 2, 3, 1, 1, 1, 2, True),
    (2, 2816, 8, 8, 3, 1, 1, 1, 8, True),
    # families of DESIGN.md section 4 the list above does not reach
    (3, 10701, 64, 64, 3, 1, 1, 1, 0, True),       # >= 500 tiles of 64x64 with K = 192 < 256: v2 / classic, ragged M (32103 rows)
    (3, 1501, 64, 160, 3, 1, 1, 1, 0, False),      # > 512 tiles of 32x32, < 500 of 64x64: `fast`, ragged M and N
    (9, 157, 256, 1536, 1, 1, 0, 1, 0, False),     # 1536-column projection on macro tiles (128x192), ragged M (1413 rows)
    (3, 45, 128, 96, 3, 1, 1, 1, 0, False),        # register-staged, a wave's K range ends inside a tap, ragged rows and clips
    (2, 353, 128, 128, 3, 1, 1, 2, 0, True),       # nearest x2 upsample in front of an MFMA convolution, odd length
]


def _conv_inputs(B, L, C, N, taps, stride, pad, up, groups, residual, td, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, L, C, generator=g) * 1.5 + 0.3).to(td)
    w = torch.randn(N, C, taps, generator=g) / (C * taps) ** 0.5
    bias = torch.randn(N, generator=g) * 0.1
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    Lout = (L * up + 2 * pad - taps) // stride + 1
    res = torch.randn(B, Lout, N, generator=g).to(td) if residual else None
    return x, w, bias, gamma, beta, res, Lout


@pytest.mark.parametrize("dtype", ["fp32", "fp32x", "bf16", "fp16"])
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_conv1d_cl(cuda, dtype, shape):
    from syncfusion_amd.autograd import conv1d_workspace_bytes

    _l, lib = _lib()
    B, L, C, N, taps, stride, pad, up, groups, residual = shape
    td = TD[dtype]
    x, w, bias, gamma, beta, res, Lout = _conv_inputs(*shape, td)
    nws = conv1d_workspace_bytes(B, C, N, taps, groups)

    def run(a):
        xs, ws_, bs = a.inp(x, "x"), a.inp(w, "w"), a.inp(bias, "bias")
        gs, bes = (a.inp(gamma, "gamma"), a.inp(beta, "beta")) if groups else (None, None)
        rs = a.inp(res, "residual") if residual else None
        out = a.out((B, Lout, N), td, "out")
        wk = a.ws(nws, "ws")
        rc = lib.sf_op_conv1d_cl(_l.DTYPES[dtype], xs.ptr, ws_.ptr, bs.ptr, _ptr(gs), _ptr(bes), groups, 1e-5, _ptr(rs), B, L, C, N, taps, stride, pad,
                                 up, out.ptr, wk.ptr, nws, _l.stream_ptr(cuda))
        return rc, [out]

    _run_case(cuda, "sf_op_conv1d_cl", run)


# ---------------------------------------------------------------------------------------------------------------------------------
# norms, attention
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("with_ws", [True, False])
@pytest.mark.parametrize("B,L,C", [(3, 44, 1024), (3, 1000, 512), (1, 4096, 256), (2, 64, 4096)])
def test_gn_silu(cuda, dtype, with_ws, B, L, C):
    _l, lib = _lib()
    G, td = 8, TD[dtype]
    g = torch.Generator().manual_seed(L + C)
    x = (torch.randn(B, L, C, generator=g) * 1.4 + 0.3).to(td)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    nws = B * 32 * G * 2 * 4       # the header's bound, in bytes

    def run(a):
        xs, gs, bs = a.inp(x, "x"), a.inp(gamma, "gamma"), a.inp(beta, "beta")
        out = a.out((B, L, C), td, "out")
        wk = a.ws(nws, "ws") if with_ws else None
        rc = lib.sf_op_gn_silu(_l.DTYPES[dtype], xs.ptr, gs.ptr, bs.ptr, G, 1e-5, B, L, C, out.ptr, _ptr(wk), nws if with_ws else 0, _l.stream_ptr(cuda))
        return rc, [out]

    _run_case(cuda, "sf_op_gn_silu", run)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("mod", [True, False])
@pytest.mark.parametrize("C", [8, 32, 1024])
def test_ln_modulate(cuda, dtype, mod, C):
    _l, lib = _lib()
    B, L, td = 3, 37, TD[dtype]
    g = torch.Generator().manual_seed(C)
    x = (torch.randn(B, L, C, generator=g) * 2 + 0.5).to(td)
    ss = torch.randn(B, 2 * C, generator=g) * 0.3

    def run(a):
        xs = a.inp(x, "x")
        sd = a.inp(ss, "scale_shift") if mod else None
        out = a.out((B, L, C), td, "out")
        return lib.sf_op_ln_modulate(_l.DTYPES[dtype], xs.ptr, _ptr(sd), 1e-6 if mod else 1e-5, B, L, C, out.ptr, _l.stream_ptr(cuda)), [out]

    _run_case(cuda, "sf_op_ln_modulate", run)


@pytest.mark.parametrize("dtype", ["fp32", "fp32x", "bf16", "fp16"])
@pytest.mark.parametrize("B,H,L", [(2, 3, 1), (2, 3, 44), (2, 3, 100), (40, 8, 300), (9, 8, 1100)])
def test_attention(cuda, dtype, B, H, L):
    _l, lib = _lib()
    D, td = 64, TD[dtype]
    g = torch.Generator().manual_seed(L + B)
    q = torch.randn(B, L, H * D, generator=g).to(td)
    kv = torch.randn(B, L, 2 * H * D, generator=g).to(td)

    def run(a):
        qs, ks = a.inp(q, "q"), a.inp(kv, "kv")
        out = a.out((B, L, H * D), td, "out")
        return lib.sf_op_attention(_l.DTYPES[dtype], qs.ptr, ks.ptr, B, L, H, D, out.ptr, _l.stream_ptr(cuda)), [out]

    _run_case(cuda, "sf_op_attention", run)


# ---------------------------------------------------------------------------------------------------------------------------------
# fused chains of the deep levels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,B,L,C,kb", [(d, *s) for s in ((5, 61, 512, 1), (4, 44, 1024, 1), (3, 61, 512, 2)) for d in ("bf16", "fp16", "fp32x")
                                            if not (d == "fp32x" and s[3] == 2)])   # (the split-operand form takes one channel block per workgroup)
def test_resnet_mod_cb(cuda, dtype, B, L, C, kb):
    _l, lib = _lib()
    G, td = 8, TD[dtype]
    g = torch.Generator().manual_seed(B * 1000 + L + C)
    x = (torch.randn(B, L, C, generator=g) * 1.3 + 0.2).to(td)
    w1 = torch.randn(C, C, 3, generator=g) / (3 * C) ** 0.5
    w2 = torch.randn(C, C, 3, generator=g) / (3 * C) ** 0.5
    b1, b2 = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    gam = [1 + 0.2 * torch.randn(C, generator=g) for _ in range(2)]
    bet = [0.1 * torch.randn(C, generator=g) for _ in range(2)]
    ss = torch.randn(B, 2 * C, generator=g) * 0.3
    nws = int(lib.sf_op_resnet_mod_cb_workspace_bytes(B, L, C))
    assert nws > 0

    def run(a):
        xs = a.inp(x, "x")
        keep = [a.inp(t, n) for t, n in ((w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2"), (gam[0], "gn1_g"), (bet[0], "gn1_b"), (gam[1], "gn2_g"),
                                         (bet[1], "gn2_b"))]
        sd = a.inp(ss, "scale_shift")
        h, m = a.out((B, L, C), td, "h_out"), a.out((B, L, C), td, "m_out")
        wk = a.ws(nws, "ws")
        rc = lib.sf_op_resnet_mod_cb(_l.DTYPES[dtype], xs.ptr, *[t.ptr for t in keep], G, 1e-5, sd.ptr, 1e-6, B, L, C, kb, h.ptr, m.ptr, wk.ptr, nws,
                                     _l.stream_ptr(cuda))
        return rc, [h, m]

    _run_case(cuda, "sf_op_resnet_mod_cb", run)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,L,C,C2,N,want_fused", [
    (7, 301, 256, 64, 384, 1),      # fused pair, ragged rows (2107 = 16 x 128 + 59), 192-wide tiles with an empty half
    (5, 1000, 128, 32, 256, 0),     # C2 = 32: falls back to z -> ln_modulate -> plain projection
    (4, 44, 1024, 256, 1536, 1),    # small batch: the 32x32 families carry the same fusion
])
def test_inject_prenorm_proj(cuda, dtype, B, L, C, C2, N, want_fused):
    _l, lib = _lib()
    td = TD[dtype]
    g = torch.Generator().manual_seed(B * 1000 + L + C)
    m = (torch.randn(B, L, C, generator=g) * 1.3 + 0.4).to(td)
    ctx = torch.randn(B, L, C2, generator=g).to(td)
    w_inj = torch.randn(C, C + C2, generator=g) / (C + C2) ** 0.5
    b_inj = torch.randn(C, generator=g) * 0.1
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    w_q = torch.randn(N, C, generator=g) / C ** 0.5
    nws = int(lib.sf_op_inject_prenorm_proj_workspace_bytes(B, L, C, C2, N))
    assert nws > 0

    def run(a):
        ms, cs = a.inp(m, "m"), a.inp(ctx, "ctx")
        p = [a.inp(t, n) for t, n in ((w_inj, "w_inj"), (b_inj, "b_inj"), (gamma, "gamma"), (beta, "beta"), (w_q, "w_q"))]
        z, q = a.out((B, L, C), td, "z_out"), a.out((B, L, N), td, "q_out")
        wk = a.ws(nws, "ws")
        fused = ct.c_int(-1)
        rc = lib.sf_op_inject_prenorm_proj(_l.DTYPES[dtype], ms.ptr, cs.ptr, p[0].ptr, p[1].ptr, p[2].ptr, p[3].ptr, 1e-5, p[4].ptr, B, L, C, C2, N,
                                           z.ptr, q.ptr, ct.byref(fused), wk.ptr, nws, _l.stream_ptr(cuda))
        assert rc != 0 or fused.value == want_fused
        return rc, [z, q]

    _run_case(cuda, "sf_op_inject_prenorm_proj", run)


# ---------------------------------------------------------------------------------------------------------------------------------
# glue, resampler, input side
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cut_prefix_crop(cuda):
    _l, lib = _lib()
    g = torch.Generator().manual_seed(11)
    B, Cc, L, Lc = 5, 2, 5000, 4410
    gen = torch.randn(B, Cc, L, generator=g)
    y = torch.zeros(B, 1, L)
    for i, f in enumerate([0, 17, 2047, 4409, 4999]):
        y[i, 0, f] = 1.0
        y[i, 0, min(L - 1, f + 300)] = 1.0

    def run(a):
        gs, ys = a.inp(gen, "gen"), a.inp(y, "y")
        out, first = a.out((B, Cc, Lc), torch.float32, "out"), a.out((B,), torch.int32, "first_onset")
        return lib.sf_cut_prefix_crop(gs.ptr, ys.ptr, B, Cc, L, Lc, out.ptr, first.ptr, _l.stream_ptr(cuda)), [out, first]

    _run_case(cuda, "sf_cut_prefix_crop", run)


@pytest.mark.parametrize("with_start", [True, False])
def test_onsets_to_track(cuda, with_start):
    _l, lib = _lib()
    g = torch.Generator().manual_seed(5)
    N, T, L = 4, 30, 60001          # onsets of the later frames fall behind the end of the track and are dropped
    logits = torch.randn(N, T, generator=g)
    start = torch.tensor([0, 30, 45, 7], dtype=torch.int32)

    def run(a):
        ls = a.inp(logits, "logits")
        st = a.inp(start, "start_frame") if with_start else None
        tr = a.out((N, 1, L), torch.float32, "track")
        return lib.sf_onsets_to_track(ls.ptr, N, T, _ptr(st), 15.0, 48000.0, 0.5, tr.ptr, L, _l.stream_ptr(cuda)), [tr]

    _run_case(cuda, "sf_onsets_to_track", run)


def test_times_to_track(cuda):
    _l, lib = _lib()
    sr, L, B = 48000.0, 96001, 4
    times = [[0.0, 0.1234, 1.99999, 2.00002], [0.5], [], [1.0000001, 2.5]]        # the last sample of the track, and two times behind its end
    flat = torch.tensor([t for ts in times for t in ts], dtype=torch.float64)
    clip = torch.tensor([b for b, ts in enumerate(times) for _ in ts], dtype=torch.int32)

    def run(a):
        ts, cs = a.inp(flat, "times"), a.inp(clip, "clip_of")
        tr = a.out((B, 1, L), torch.float32, "track")
        return lib.sf_times_to_track(ts.ptr, cs.ptr, flat.numel(), sr, B, L, tr.ptr, _l.stream_ptr(cuda)), [tr]

    _run_case(cuda, "sf_times_to_track", run)


def test_resampler_forward(cuda):
    _l, lib = _lib()
    R, L = 3, 1001
    x = torch.randn(R, L, generator=torch.Generator().manual_seed(L))
    h = ct.c_void_p()
    _l.check(lib.sf_resampler_create(48000, 22050, 6, 0.99, ct.byref(h)), "sf_resampler_create")
    try:
        Lout = int(lib.sf_resampler_out_length(h, L))
        assert Lout == -(-22050 * L // 48000)

        def run(a):
            xs = a.inp(x, "x")
            out = a.out((R, Lout), torch.float32, "out")
            return lib.sf_resampler_forward(h, xs.ptr, R, L, out.ptr, _l.stream_ptr(cuda)), [out]

        _run_case(cuda, "sf_resampler_forward", run)
    finally:
        torch.cuda.synchronize()
        lib.sf_resampler_destroy(h)


MEAN, STD = (0.43216, 0.394666, 0.37645), (0.22803, 0.22145, 0.216989)


def test_frames_preprocess(cuda):
    _l, lib = _lib()
    N, T, H, W, oh, ow = 3, 4, 100, 130, 112, 112
    fr = torch.randint(0, 256, (N, T, H, W, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    m, s = (ct.c_float * 3)(*MEAN), (ct.c_float * 3)(*STD)

    def run(a):
        fs = a.inp(fr, "frames", ld=W * 3)
        out = a.out((N, 3, T, oh, ow), torch.float32, "out")
        return lib.sf_frames_preprocess(fs.ptr, N, T, H, W, oh, ow, m, s, out.ptr, _l.stream_ptr(cuda)), [out]

    _run_case(cuda, "sf_frames_preprocess", run)


@pytest.mark.parametrize("contrast", [True, False])
def test_frames_augment(cuda, contrast):
    """uint8 input: the NaN trick does not apply to reads past it; the checks are the write guards and bit equality with the plain run."""
    from syncfusion_amd.frame_transforms import ClipParams

    _l, lib = _lib()
    N, T, H, W, rh, rw, oh, ow = 3, 2, 61, 83, 45, 57, 37, 41
    fr = torch.randint(0, 256, (N, T, H, W, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    mask = 0b1101 | (2 if contrast else 0)
    cp = ClipParams((rh, rw), (oh, ow), torch.tensor([0, 8, 3], dtype=torch.int32), torch.tensor([16, 0, 5], dtype=torch.int32),
                    torch.tensor([[0, 1, 2, 3], [3, 1, 0, 2], [2, 3, 1, 0]], dtype=torch.int32),
                    torch.tensor([[1.2, 0.7, 1.3, 0.1], [0.8, 1.4, 0.6, -0.2], [1.0, 1.1, 0.9, 0.05]]), torch.tensor([mask, mask, 0], dtype=torch.int32))
    host = cp.table().contiguous()
    m, s = (ct.c_float * 3)(*MEAN), (ct.c_float * 3)(*STD)
    nws = int(lib.sf_frames_augment_workspace_bytes(N, T, oh, ow))
    assert nws >= 0

    def run(a):
        fs, tab = a.inp(fr, "frames", ld=W * 3), a.inp(host, "table_dev")
        out = a.out((N, 3, T, oh, ow), torch.float32, "out")
        wk = a.ws(nws, "ws")
        rc = lib.sf_frames_augment(fs.ptr, N, T, H, W, rh, rw, oh, ow, host.data_ptr(), tab.ptr, m, s, out.ptr, wk.ptr, nws, _l.stream_ptr(cuda))
        return rc, [out]

    _run_case(cuda, "sf_frames_augment", run)


# ---------------------------------------------------------------------------------------------------------------------------------
# training entries
# ---------------------------------------------------------------------------------------------------------------------------------
TRAIN_CONV = [(3, 100, 128, 128, 3, 8), (3, 700, 256, 256, 3, 8), (1, 9, 32, 32, 3, 8), (2, 704, 40, 32, 1, 0), (1, 77, 33, 17, 3, 0), (2, 2816, 8, 8, 3, 8),
              (2, 1024, 64, 64, 3, 8)]


def _train_conv_inputs(B, L, C, N, taps, groups):
    g = torch.Generator().manual_seed(B * 1000 + L + C)
    x = torch.randn(B, L, C, generator=g) * 1.3 + 0.2
    w = torch.randn(N, C, taps, generator=g) / (C * taps) ** 0.5
    b = torch.randn(N, generator=g) * 0.1
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    dy = torch.randn(B, L, N, generator=g)
    res = torch.randn(B, L, N, generator=g)
    add = torch.randn(B, L, C, generator=g)
    return x, w, b, gamma, beta, dy, res, add


@pytest.mark.parametrize("dtype", ["fp32", "fp32x"])
@pytest.mark.parametrize("B,L,C,N,taps,groups", TRAIN_CONV)
def test_conv1d_train_fwd(cuda, dtype, B, L, C, N, taps, groups):
    from syncfusion_amd.autograd import conv1d_workspace_bytes

    _l, lib = _lib()
    x, w, b, gamma, beta, dy, res, add = _train_conv_inputs(B, L, C, N, taps, groups)
    nws = conv1d_workspace_bytes(B, C, N, taps, groups)
    npk = int(lib.sf_op_conv1d_dgrad_pack_bytes(C, N, taps))
    assert npk == 8 * C * N * taps

    def run(a):
        xs, ws_, bs, rs = a.inp(x, "x"), a.inp(w, "w"), a.inp(b, "bias"), a.inp(res, "residual")
        gs, bes = (a.inp(gamma, "gamma"), a.inp(beta, "beta")) if groups else (None, None)
        out = a.out((B, L, N), torch.float32, "out")
        pk = a.ws(npk, "dgrad_pack", ld=4 * N)
        wk = a.ws(nws, "ws")
        rc = lib.sf_op_conv1d_train_fwd(_l.DTYPES[dtype], xs.ptr, ws_.ptr, bs.ptr, _ptr(gs), _ptr(bes), groups, 1e-5, rs.ptr, B, L, C, N, taps, taps // 2,
                                        out.ptr, pk.ptr, npk, wk.ptr, nws, _l.stream_ptr(cuda))
        return rc, [out]

    _run_case(cuda, "sf_op_conv1d_train_fwd", run)


@pytest.mark.parametrize("B,L,C", [(3, 100, 128), (3, 700, 256), (1, 9, 32), (2, 2816, 8), (2, 1024, 64)])
def test_gn_silu_train(cuda, B, L, C):
    """(the entry takes no dtype: fp32 only)"""
    _l, lib = _lib()
    G = 8
    x, _, _, gamma, beta, _, _, _ = _train_conv_inputs(B, L, C, C, 3, G)
    nst = int(lib.sf_op_gn_silu_train_stats_floats(B, L, C, G))
    assert nst >= 0

    def run(a):
        xs, gs, bs = a.inp(x, "x"), a.inp(gamma, "gamma"), a.inp(beta, "beta")
        act = a.out((B, L, C), torch.float32, "act")
        st = a.out((nst,), torch.float32, "stats")
        rc = lib.sf_op_gn_silu_train(xs.ptr, gs.ptr, bs.ptr, G, 1e-5, B, L, C, act.ptr, st.ptr if nst else None, _l.stream_ptr(cuda))
        return rc, [act, st] if nst else [act]

    _run_case(cuda, "sf_op_gn_silu_train", run)


@pytest.mark.parametrize("dtype", ["fp32", "fp32x"])
@pytest.mark.parametrize("saved", ["all", "none"])       # with / without dgrad_pack, act, stats and dx_add
@pytest.mark.parametrize("B,L,C,N,taps,groups", TRAIN_CONV)
def test_conv1d_bwd_cl_p(cuda, dtype, saved, B, L, C, N, taps, groups):
    from syncfusion_amd.autograd import conv1d_workspace_bytes

    _l, lib = _lib()
    x, w, b, gamma, beta, dy, res, add = _train_conv_inputs(B, L, C, N, taps, groups)
    dt, pad, st = _l.DTYPES[dtype], taps // 2, _l.stream_ptr(cuda)
    nws = int(lib.sf_op_conv1d_bwd_workspace_bytes(B, L, C, N, taps, groups))
    assert nws >= 0
    want_dx = not (N % 32 != 0 and C > 32)      # (the data gradient of a thin output over wide inputs is not supported)
    # the forward pass's products the backward pass reads, made once on ordinary allocations
    dev = lambda t: t.to(cuda)   # noqa: E731
    act_t = stats_t = pack_t = None
    if saved == "all":
        xd, wd, bd = dev(x), dev(w), dev(b)
        if groups:
            nst = int(lib.sf_op_gn_silu_train_stats_floats(B, L, C, groups))
            act_t = torch.empty(B, L, C, device=cuda)
            stats_t = torch.empty(nst, device=cuda) if nst else None
            gd, bed = dev(gamma), dev(beta)
            _l.check(lib.sf_op_gn_silu_train(xd.data_ptr(), gd.data_ptr(), bed.data_ptr(), groups, 1e-5, B, L, C, act_t.data_ptr(),
                                             stats_t.data_ptr() if nst else None, st), "sf_op_gn_silu_train")
        npk = int(lib.sf_op_conv1d_dgrad_pack_bytes(C, N, taps))
        pack_t = torch.empty(npk, dtype=torch.uint8, device=cuda)
        o = torch.empty(B, L, N, device=cuda)
        nfw = conv1d_workspace_bytes(B, C, N, taps, 0)
        wsf = torch.empty(nfw, dtype=torch.uint8, device=cuda)
        src = act_t if act_t is not None else xd
        _l.check(lib.sf_op_conv1d_train_fwd(dt, src.data_ptr(), wd.data_ptr(), bd.data_ptr(), None, None, 0, 1e-5, None, B, L, C, N, taps, pad, o.data_ptr(),
                                            pack_t.data_ptr(), npk, wsf.data_ptr(), nfw, st), "sf_op_conv1d_train_fwd")
        torch.cuda.synchronize()

    def run(a):
        xs, ws_, dys = a.inp(x, "x"), a.inp(w, "w"), a.inp(dy, "dy")
        gs, bes = (a.inp(gamma, "gamma"), a.inp(beta, "beta")) if groups else (None, None)
        acts = a.inp(act_t, "act") if act_t is not None else None
        sts = a.inp(stats_t, "stats") if stats_t is not None else None
        pks = a.inp(pack_t, "dgrad_pack", ld=4 * N) if pack_t is not None else None
        adds = a.inp(add, "dx_add") if saved == "all" and groups else None
        dx = a.out((B, L, C), torch.float32, "dx") if want_dx else None
        dw, db = a.out((N, C, taps), torch.float32, "dw"), a.out((N,), torch.float32, "db")
        dgb = a.out((2 * C,), torch.float32, "dgb") if groups else None
        wk = a.ws(nws, "ws")
        rc = lib.sf_op_conv1d_bwd_cl_p(dt, xs.ptr, _ptr(acts), _ptr(sts), ws_.ptr, _ptr(pks), _ptr(gs), _ptr(bes), groups, 1e-5, dys.ptr, _ptr(adds), B, L, C,
                                       N, taps, pad, _ptr(dx), dw.ptr, db.ptr, _ptr(dgb), wk.ptr, nws, st)
        return rc, [t for t in (dx, dw, db, dgb) if t is not None]

    _run_case(cuda, "sf_op_conv1d_bwd_cl_p", run)


@pytest.mark.parametrize("entry", ["sf_op_ln_modulate_bwd", "sf_op_ln_modulate_bwd_add"])
@pytest.mark.parametrize("B,L,C", [(3, 100, 256), (1, 1, 128), (2, 300, 8), (2, 5000, 128), (1, 130, 512)])
def test_ln_modulate_bwd(cuda, entry, B, L, C):
    _l, lib = _lib()
    g = torch.Generator().manual_seed(L + C)
    x = torch.randn(B, L, C, generator=g) * 1.7 + 0.3
    ss = 0.3 * torch.randn(B, 2 * C, generator=g)
    dy, add = torch.randn(B, L, C, generator=g), torch.randn(B, L, C, generator=g)
    nws = int(lib.sf_op_ln_modulate_bwd_workspace_bytes(B, L, C))
    assert nws >= 0

    def run(a):
        xs, sd, dys = a.inp(x, "x"), a.inp(ss, "scale_shift"), a.inp(dy, "dy")
        dx, dss = a.out((B, L, C), torch.float32, "dx"), a.out((B, 2 * C), torch.float32, "dss")
        if entry.endswith("_add"):
            ad = a.inp(add, "dx_add")
            wk = a.ws(nws, "ws")
            rc = lib.sf_op_ln_modulate_bwd_add(xs.ptr, sd.ptr, dys.ptr, ad.ptr, 1e-6, B, L, C, dx.ptr, dss.ptr, wk.ptr, nws, _l.stream_ptr(cuda))
        else:
            wk = a.ws(nws, "ws")
            rc = lib.sf_op_ln_modulate_bwd(xs.ptr, sd.ptr, dys.ptr, 1e-6, B, L, C, dx.ptr, dss.ptr, wk.ptr, nws, _l.stream_ptr(cuda))
        return rc, [dx, dss]

    _run_case(cuda, entry, run)


@pytest.mark.parametrize("with_y", [True, False])
@pytest.mark.parametrize("B,L,C", [(2, 999, 3), (3, 501, 96), (2, 513, 16), (1, 1, 128)])
def test_length_sums(cuda, with_y, B, L, C):
    _l, lib = _lib()
    g = torch.Generator().manual_seed(B * 1000 + L + C)
    x, y = torch.randn(B, L, C, generator=g), torch.randn(B, L, C, generator=g)
    nws = int(lib.sf_op_length_sums_workspace_bytes(B, L, C))
    assert nws >= 0

    def run(a):
        xs = a.inp(x, "x")
        ys = a.inp(y, "y") if with_y else None
        out = a.out((B, C), torch.float32, "out")
        wk = a.ws(nws, "ws")
        return lib.sf_op_length_sums(xs.ptr, _ptr(ys), B, L, C, out.ptr, wk.ptr, nws, _l.stream_ptr(cuda)), [out]

    _run_case(cuda, "sf_op_length_sums", run)


@pytest.mark.parametrize("dtype", ["fp32", "fp32x"])
@pytest.mark.parametrize("B,L,H", [(2, 17, 3), (2, 100, 2), (3, 1, 4), (1, 2500, 1)])
def test_attention_fwd_bwd_lse(cuda, dtype, B, L, H):
    """lse is exactly B * H * L floats; the backward workspace is the smallest the entry accepts, B * H * L * 4 bytes
    (capi_train.cpp attention_bwd_lse_impl: `need`)."""
    _l, lib = _lib()
    D, dt, st = 64, _l.DTYPES[dtype], _l.stream_ptr(cuda)
    g = torch.Generator().manual_seed(L * 10 + H)
    q = torch.randn(B, L, H * D, generator=g)
    kv = torch.randn(B, L, 2 * H * D, generator=g)
    do = torch.randn(B, L, H * D, generator=g)

    def fwd(a):
        qs, ks = a.inp(q, "q"), a.inp(kv, "kv")
        out, lse = a.out((B, L, H * D), torch.float32, "out"), a.out((B * H * L,), torch.float32, "lse")
        return lib.sf_op_attention_fwd_lse_x(dt, qs.ptr, ks.ptr, B, L, H, D, out.ptr, lse.ptr, st), [out, lse]

    _run_case(cuda, "sf_op_attention_fwd_lse_x", fwd)
    p = Plain(cuda)
    rc, (o_t, lse_t) = fwd(p)
    assert rc == 0
    torch.cuda.synchronize()
    nws = B * H * L * 4
    assert lib.sf_op_attention_bwd_lse_x(dt, o_t.ptr, o_t.ptr, o_t.ptr, o_t.ptr, lse_t.ptr, B, L, H, D, o_t.ptr, o_t.ptr, o_t.ptr, nws - 1, st) != 0, \
        "one byte less is refused (nothing is launched)"

    def bwd(a):
        qs, ks, os_, dos, ls = a.inp(q, "q"), a.inp(kv, "kv"), a.inp(o_t.payload, "out"), a.inp(do, "dout"), a.inp(lse_t.payload, "lse")
        dq, dkv = a.out((B, L, H * D), torch.float32, "dq"), a.out((B, L, 2 * H * D), torch.float32, "dkv")
        wk = a.ws(nws, "ws")
        rc = lib.sf_op_attention_bwd_lse_x(dt, qs.ptr, ks.ptr, os_.ptr, dos.ptr, ls.ptr, B, L, H, D, dq.ptr, dkv.ptr, wk.ptr, nws, st)
        return rc, [dq, dkv]

    _run_case(cuda, "sf_op_attention_bwd_lse_x", bwd)


# ---------------------------------------------------------------------------------------------------------------------------------
# onset training entries
# ---------------------------------------------------------------------------------------------------------------------------------
VCONV = [
    # name, cin, cin_ld, cout, kernel, stride, padding, N, T, H, W   (two odd-extent geometries of CONV_CASES in test_gpu_onset_train.py)
    ("stem", 3, 4, 45, (1, 7, 7), 2, (0, 3, 3), 2, 2, 15, 9),                 # cin_ld 4 > cin 3
    ("temporal45", 45, 64, 64, (3, 1, 1), 1, (1, 0, 0), 2, 5, 7, 9),          # cin_ld 64 > cin 45
    ("spatial_s2_230", 64, 64, 230, (1, 3, 3), 2, (0, 1, 1), 2, 2, 15, 9),    # cout_ld 256 > cout 230, stride 2 over odd frames
]


def _rows(x, ld):
    N, Cc, T, H, W = x.shape
    r = torch.zeros(N * T * H * W, ld, dtype=x.dtype)
    r[:, :Cc] = x.permute(0, 2, 3, 4, 1).reshape(-1, Cc)
    return r


@pytest.mark.parametrize("case", VCONV, ids=[c[0] for c in VCONV])
def test_vconv_fwd_bwd(cuda, case):
    from syncfusion_amd.onset_training import row_ld

    _l, lib = _lib()
    name, cin, cin_ld, cout, k, s, p, N, T, H, W = case
    assert cin_ld == row_ld(cin)
    cout_ld = row_ld(cout)
    Ho, Wo = (H + 2 * p[1] - k[1]) // s + 1, (W + 2 * p[2] - k[2]) // s + 1
    d = _l.VConvDesc(N, T, H, W, cin, cin_ld, cout, cout_ld, k[0], k[1], k[2], s, s, p[0], p[1], p[2])
    g = torch.Generator().manual_seed(11)
    w = torch.randn(cout, cin, *k, generator=g) / (cin * k[0] * k[1] * k[2]) ** 0.5
    x = _rows(torch.randn(N, cin, T, H, W, generator=g), cin_ld)
    dy = _rows(torch.randn(N, cout, T, Ho, Wo, generator=g), cout_ld)
    nws = int(lib.sf_op_vconv_workspace_bytes(ct.byref(d)))
    assert nws >= 0
    st = _l.stream_ptr(cuda)

    def fwd(a):
        xs, ws_ = a.inp(x, "x"), a.inp(w, "w", ld=cin * k[0] * k[1] * k[2])
        y = a.out((N * T * Ho * Wo, cout_ld), torch.float32, "y")
        wk = a.ws(nws, "ws")
        return lib.sf_op_vconv_fwd(ct.byref(d), xs.ptr, ws_.ptr, y.ptr, wk.ptr, nws, st), [y]

    _run_case(cuda, "sf_op_vconv_fwd", fwd)

    def bwd(a):
        xs, ws_, dys = a.inp(x, "x"), a.inp(w, "w", ld=cin * k[0] * k[1] * k[2]), a.inp(dy, "dy")
        dx = a.out((N * T * H * W, cin_ld), torch.float32, "dx")
        dw = a.out(tuple(w.shape), torch.float32, "dw", ld=cin * k[0] * k[1] * k[2])
        wk = a.ws(nws, "ws")
        return lib.sf_op_vconv_bwd(ct.byref(d), xs.ptr, ws_.ptr, dys.ptr, dx.ptr, dw.ptr, wk.ptr, nws, st), [dx, dw]

    _run_case(cuda, "sf_op_vconv_bwd", bwd)


def _bn_inputs(rows, Cc, ld, seed=5):
    g = torch.Generator().manual_seed(seed)
    pad = lambda t: torch.cat([t, torch.zeros(rows, ld - Cc)], dim=1)   # noqa: E731
    x = pad(torch.randn(rows, Cc, generator=g) * 1.5 + 0.4)
    res, dy = pad(torch.randn(rows, Cc, generator=g)), pad(torch.randn(rows, Cc, generator=g))
    gamma, beta = 1 + 0.2 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    rm, rv = 0.1 * torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    return x, res, dy, gamma, beta, rm, rv


@pytest.mark.parametrize("rows,Cc,ld,relu,with_res", [(2 * 3 * 5 * 7, 45, 64, 1, True), (1001, 230, 256, 0, False), (2, 3, 4, 1, False)])
def test_bn_train_fwd_bwd(cuda, rows, Cc, ld, relu, with_res):
    _l, lib = _lib()
    x, res, dy, gamma, beta, rm, rv = _bn_inputs(rows, Cc, ld)
    nws = int(lib.sf_op_bn_train_workspace_bytes(rows, Cc))
    assert nws >= 0
    st = _l.stream_ptr(cuda)
    nbt = torch.zeros(1, dtype=torch.int64)

    def fwd(a):
        xs, gs, bs = a.inp(x, "x"), a.inp(gamma, "gamma"), a.inp(beta, "beta")
        rs = a.inp(res, "res") if with_res else None
        rms, rvs, nb = a.inout(rm, "running_mean"), a.inout(rv, "running_var"), a.inout(nbt, "num_batches_tracked")
        y = a.out((rows, ld), torch.float32, "y")
        mean, inv = a.out((Cc,), torch.float32, "save_mean"), a.out((Cc,), torch.float32, "save_invstd")
        wk = a.ws(nws, "ws")
        rc = lib.sf_op_bn_train_fwd(xs.ptr, _ptr(rs), rows, Cc, ld, gs.ptr, bs.ptr, 1e-5, 0.1, rms.ptr, rvs.ptr, nb.ptr, relu, y.ptr, mean.ptr, inv.ptr,
                                    wk.ptr, nws, st)
        return rc, [y, mean, inv, rms, rvs, nb]

    _run_case(cuda, "sf_op_bn_train_fwd", fwd)
    p = Plain(cuda)
    rc, (y_t, mean_t, inv_t, _, _, _) = fwd(p)
    assert rc == 0
    torch.cuda.synchronize()

    def bwd(a):
        xs, dys, gs = a.inp(x, "x"), a.inp(dy, "dy"), a.inp(gamma, "gamma")
        ys = a.inp(y_t.payload, "y") if relu else None
        ms, iv = a.inp(mean_t.payload, "save_mean"), a.inp(inv_t.payload, "save_invstd")
        dx = a.out((rows, ld), torch.float32, "dx")
        dres = a.out((rows, ld), torch.float32, "dres") if with_res else None
        dg, db = a.out((Cc,), torch.float32, "dgamma"), a.out((Cc,), torch.float32, "dbeta")
        wk = a.ws(nws, "ws")
        rc = lib.sf_op_bn_train_bwd(xs.ptr, _ptr(ys), dys.ptr, rows, Cc, ld, gs.ptr, ms.ptr, iv.ptr, dx.ptr, _ptr(dres), dg.ptr, db.ptr, wk.ptr, nws, st)
        return rc, [t for t in (dx, dres, dg, db) if t is not None]

    _run_case(cuda, "sf_op_bn_train_bwd", bwd)


@pytest.mark.parametrize("rows,Cc,ld,relu,with_res", [(2 * 3 * 5 * 7, 45, 64, 1, True), (1001, 230, 256, 0, False), (1, 3, 4, 1, False)])
def test_bn_sync(cuda, rows, Cc, ld, relu, with_res):
    """The four split-phase calls as one rank of a world of two: the other rank's table rows are this rank's numbers shifted."""
    _l, lib = _lib()
    x, res, dy, gamma, beta, rm, rv = _bn_inputs(rows, Cc, ld, seed=6)
    nws = int(lib.sf_op_bn_sync_workspace_bytes(rows, Cc))
    assert nws >= 0
    st = _l.stream_ptr(cuda)
    world = 2
    counts = torch.tensor([rows, rows + 3], dtype=torch.int64)
    nbt = torch.zeros(1, dtype=torch.int64)

    def stats(a):
        xs = a.inp(x, "x")
        loc = a.out((Cc, 2), torch.float32, "local_stats")
        wk = a.ws(nws, "ws")
        return lib.sf_op_bn_sync_stats(xs.ptr, rows, Cc, ld, loc.ptr, wk.ptr, nws, st), [loc]

    _run_case(cuda, "sf_op_bn_sync_stats", stats)
    rc, (loc_t,) = stats(Plain(cuda))
    assert rc == 0
    torch.cuda.synchronize()
    other = loc_t.payload.clone()
    other[:, 0] += 0.25
    other[:, 1] = other[:, 1] * 1.1 + 0.5
    table = torch.stack([loc_t.payload, other])

    def fwd(a):
        xs, gs, bs, tb, cn = a.inp(x, "x"), a.inp(gamma, "gamma"), a.inp(beta, "beta"), a.inp(table, "gathered_stats"), a.inp(counts, "row_counts")
        rs = a.inp(res, "res") if with_res else None
        rms, rvs, nb = a.inout(rm, "running_mean"), a.inout(rv, "running_var"), a.inout(nbt, "num_batches_tracked")
        y = a.out((rows, ld), torch.float32, "y")
        mean, inv = a.out((Cc,), torch.float32, "save_mean"), a.out((Cc,), torch.float32, "save_invstd")
        wk = a.ws(nws, "ws")
        rc = lib.sf_op_bn_sync_fwd_apply(xs.ptr, _ptr(rs), rows, Cc, ld, tb.ptr, cn.ptr, world, gs.ptr, bs.ptr, 1e-5, 0.1, rms.ptr, rvs.ptr, nb.ptr, relu,
                                         y.ptr, mean.ptr, inv.ptr, wk.ptr, nws, st)
        return rc, [y, mean, inv, rms, rvs, nb]

    _run_case(cuda, "sf_op_bn_sync_fwd_apply", fwd)
    rc, (y_t, mean_t, inv_t, _, _, _) = fwd(Plain(cuda))
    assert rc == 0
    torch.cuda.synchronize()

    def sums(a):
        xs, dys = a.inp(x, "x"), a.inp(dy, "dy")
        ys = a.inp(y_t.payload, "y") if relu else None
        ms, iv = a.inp(mean_t.payload, "save_mean"), a.inp(inv_t.payload, "save_invstd")
        loc = a.out((Cc, 2), torch.float32, "local_sums")
        dg, db = a.out((Cc,), torch.float32, "dgamma"), a.out((Cc,), torch.float32, "dbeta")
        wk = a.ws(nws, "ws")
        rc = lib.sf_op_bn_sync_bwd_sums(xs.ptr, _ptr(ys), dys.ptr, rows, Cc, ld, ms.ptr, iv.ptr, loc.ptr, dg.ptr, db.ptr, wk.ptr, nws, st)
        return rc, [loc, dg, db]

    _run_case(cuda, "sf_op_bn_sync_bwd_sums", sums)
    rc, (sums_t, _, _) = sums(Plain(cuda))
    assert rc == 0
    torch.cuda.synchronize()
    gathered = torch.stack([sums_t.payload, sums_t.payload * 0.9 + 0.1])

    def apply(a):
        xs, dys, gs, tb, cn = a.inp(x, "x"), a.inp(dy, "dy"), a.inp(gamma, "gamma"), a.inp(gathered, "gathered_sums"), a.inp(counts, "row_counts")
        ys = a.inp(y_t.payload, "y") if relu else None
        ms, iv = a.inp(mean_t.payload, "save_mean"), a.inp(inv_t.payload, "save_invstd")
        dx = a.out((rows, ld), torch.float32, "dx")
        dres = a.out((rows, ld), torch.float32, "dres") if with_res else None
        wk = a.ws(nws, "ws")
        rc = lib.sf_op_bn_sync_bwd_apply(xs.ptr, _ptr(ys), dys.ptr, rows, Cc, ld, tb.ptr, cn.ptr, world, gs.ptr, ms.ptr, iv.ptr, dx.ptr, _ptr(dres), wk.ptr,
                                         nws, st)
        return rc, [t for t in (dx, dres) if t is not None]

    _run_case(cuda, "sf_op_bn_sync_bwd_apply", apply)


@pytest.mark.parametrize("N,Cc,T,H,W,ld", [(2, 3, 3, 9, 7, 4), (1, 3, 1, 1, 1, 4), (2, 45, 2, 5, 3, 64)])
def test_video_to_cl(cuda, N, Cc, T, H, W, ld):
    _l, lib = _lib()
    x = torch.randn(N, Cc, T, H, W, generator=torch.Generator().manual_seed(2))

    def run(a):
        xs = a.inp(x, "x")
        out = a.out((N * T * H * W, ld), torch.float32, "out")
        return lib.sf_op_video_to_cl(xs.ptr, N, Cc, T, H, W, ld, out.ptr, _l.stream_ptr(cuda)), [out]

    _run_case(cuda, "sf_op_video_to_cl", run)


@pytest.mark.parametrize("NT,HW,Cc,ld", [(7, 35, 512, 512), (3, 1, 45, 64), (1, 63, 230, 256)])
def test_video_pool_fwd_bwd(cuda, NT, HW, Cc, ld):
    _l, lib = _lib()
    g = torch.Generator().manual_seed(NT + HW)
    x = torch.cat([torch.randn(NT * HW, Cc, generator=g), torch.zeros(NT * HW, ld - Cc)], dim=1)
    dout = torch.randn(NT, Cc, generator=g)

    def fwd(a):
        xs = a.inp(x, "x")
        out = a.out((NT, Cc), torch.float32, "out")
        return lib.sf_op_video_pool(xs.ptr, NT, HW, Cc, ld, out.ptr, _l.stream_ptr(cuda)), [out]

    def bwd(a):
        ds = a.inp(dout, "dout")
        dx = a.out((NT * HW, ld), torch.float32, "dx")
        return lib.sf_op_video_pool_bwd(ds.ptr, NT, HW, Cc, ld, dx.ptr, _l.stream_ptr(cuda)), [dx]

    _run_case(cuda, "sf_op_video_pool", fwd)
    _run_case(cuda, "sf_op_video_pool_bwd", bwd)


@pytest.mark.parametrize("N,T", [(7, 43), (1, 1), (3, 256)])      # n = 301 (not a multiple of 256), n = 1, n = 768
def test_onset_loss_entries(cuda, N, T):
    _l, lib = _lib()
    n = N * T
    g = torch.Generator().manual_seed(n)
    z = torch.randn(n, generator=g) * 2
    t = (torch.rand(n, generator=g) < 0.3).float()
    t[0] = 1.0            # n = 1: the only label is a positive (pos_weight 0, a finite loss); otherwise both classes are present
    if n > 1:
        t[-1] = 0.0
    up = torch.tensor([0.7])
    nws = int(lib.sf_op_onset_loss_workspace_bytes(n))
    assert nws >= 0
    st = _l.stream_ptr(cuda)

    def fwd(a):
        zs, ts = a.inp(z, "z"), a.inp(t, "t")
        loss, stats = a.out((1,), torch.float32, "loss"), a.out((2,), torch.float32, "stats")
        wk = a.ws(nws, "ws")
        return lib.sf_op_onset_bce_fwd(zs.ptr, ts.ptr, n, loss.ptr, stats.ptr, wk.ptr, nws, st), [loss, stats]

    _run_case(cuda, "sf_op_onset_bce_fwd", fwd)
    rc, (_, stats_t) = fwd(Plain(cuda))
    assert rc == 0
    torch.cuda.synchronize()

    def bwd(a):
        zs, ts, ss, gs = a.inp(z, "z"), a.inp(t, "t"), a.inp(stats_t.payload, "stats"), a.inp(up, "g")
        dz = a.out((n,), torch.float32, "dz")
        return lib.sf_op_onset_bce_bwd(zs.ptr, ts.ptr, ss.ptr, gs.ptr, n, dz.ptr, st), [dz]

    _run_case(cuda, "sf_op_onset_bce_bwd", bwd)

    def metrics(a):
        zs, ts = a.inp(z, "z"), a.inp(t, "t")
        out = a.out((3,), torch.float64, "metrics")
        wk = a.ws(nws, "ws")
        return lib.sf_op_onset_metrics(zs.ptr, ts.ptr, N, T, 0.75, out.ptr, wk.ptr, nws, st), [out]

    if n == 1:      # one class only: AP = Acc = NaN by contract (include/syncfusion_amd.h); OnsNumAcc is a number
        plain = Plain(cuda)
        rc, (o,) = metrics(plain)
        assert rc == 0
        gd = _G(cuda)
        rc, (q,) = metrics(gd)
        assert rc == 0
        gd.verify_all()
        assert bool(torch.isnan(q.payload[:2]).all()) and bool(torch.isfinite(q.payload[2]))
        assert torch.equal(_bytes(o.payload), _bytes(q.payload))
    else:
        _run_case(cuda, "sf_op_onset_metrics", metrics)


def test_optim_adamw_step(cuda):
    """Tensors of 1, 16383, 16384 and 16385 elements (one chunk is 16384), clipping on; p, g, m and v of every tensor in guards of their own.
    g is an input (the clipped gradient is not written back); p, m, v and step are updated in place and compared with the plain run."""
    from syncfusion_amd.optim import build_table

    _l, lib = _lib()
    sizes = [1, 16383, 16384, 16385]
    g = torch.Generator().manual_seed(9)
    P = [torch.randn(n, generator=g) for n in sizes]
    Gr = [torch.randn(n, generator=g) * 3 for n in sizes]
    M = [torch.randn(n, generator=g) * 0.1 for n in sizes]
    V = [torch.rand(n, generator=g) * 0.01 for n in sizes]
    steps = [torch.tensor([float(i)]) for i in range(len(sizes))]
    hyper = torch.zeros(2 * 8, dtype=torch.float64)
    hyper[0] = 1.0                                                # max_norm: the gradients' norm is far above it
    hyper[8:13] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 1e-2], dtype=torch.float64)
    st = _l.stream_ptr(cuda)

    def run(a):
        ps = [a.inout(t, f"p{i}") for i, t in enumerate(P)]
        gs = [a.inp(t, f"g{i}") for i, t in enumerate(Gr)]
        ms = [a.inout(t, f"m{i}") for i, t in enumerate(M)]
        vs = [a.inout(t, f"v{i}") for i, t in enumerate(V)]
        ss = [a.inout(t, f"step{i}") for i, t in enumerate(steps)]
        table, total = build_table([(ps[i].ptr, gs[i].ptr, ms[i].ptr, vs[i].ptr, ss[i].ptr, n, 0) for i, n in enumerate(sizes)])
        assert total == 1 + 1 + 1 + 2
        tb, hy = a.inp(table, "desc"), a.inp(hyper, "hyper")
        res = a.out((2,), torch.float32, "result")
        nws = int(lib.sf_optim_workspace_bytes(total))
        assert nws >= 0
        wk = a.ws(nws, "ws")
        rc = lib.sf_optim_adamw_step(tb.ptr, len(sizes), total, hy.ptr, 1, 1, res.ptr, wk.ptr, nws, st)
        return rc, [res] + ps + ms + vs + ss

    _run_case(cuda, "sf_optim_adamw_step", run)


# ---------------------------------------------------------------------------------------------------------------------------------
# engines
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unet(cuda):
    return small_unet_module().to(cuda)


def _unet_args(a, x, sigma, emb, chans):
    xs = a.inp(x, "x")
    sg = a.inp(sigma, "sigma") if sigma is not None else None
    es = a.inp(emb, "emb")
    cs = [a.inp(c, f"ctx{d}") for d, c in enumerate(chans)]
    arr = (ct.c_void_p * len(cs))(*[c.ptr for c in cs])
    return xs, sg, es, cs, arr


@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("B,L0", [(1, 16), (3, 112)])
def test_unet_engine_forward(cuda, unet, B, L0, scale):
    _l, lib = _lib()
    eng = unet.engine()
    x, sigma, emb, chans = synth_inputs(SMALL_UNET, B, L0, seed=3)
    plain = eng.forward(x.to(cuda), sigma.to(cuda), [c.to(cuda) for c in chans], emb.to(cuda), scale)
    torch.cuda.synchronize()
    nws = int(lib.sf_unet_workspace_bytes(eng.handle, B, L0, int(scale != 1.0)))
    assert nws > 0
    g = _G(cuda)
    xs, sg, es, cs, arr = _unet_args(g, x, sigma, emb, chans)
    out = g.out(tuple(x.shape), torch.float32, "out")
    wk = g.ws(nws, "ws")
    rc = lib.sf_unet_forward(eng.handle, xs.ptr, sg.ptr, arr, es.ptr, B, L0, scale, out.ptr, wk.ptr, nws, _l.stream_ptr(cuda))
    assert rc == 0, lib.sf_last_error().decode()
    g.verify_all()
    assert bool(torch.isfinite(out.payload).all())
    assert torch.equal(_bytes(out.payload), _bytes(plain))


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graphed"])
def test_unet_engine_sample(cuda, unet, use_graph):
    _l, lib = _lib()
    eng = unet.engine()
    B, L0, steps, scale = 3, 112, 3, 2.0
    x, _, emb, chans = synth_inputs(SMALL_UNET, B, L0, seed=4)
    plain = eng.sample(x.to(cuda), steps, [c.to(cuda) for c in chans], emb.to(cuda), scale, use_graph=use_graph)
    torch.cuda.synchronize()
    nws = int(lib.sf_vsample_workspace_bytes(eng.handle, B, L0, 1, steps))
    assert nws > 0
    g = _G(cuda)
    _, _, es, cs, arr = _unet_args(g, x, None, emb, chans)
    g.items.pop(0)                      # (x is the in/out buffer below, not an input)
    xio = g.inout(x, "x_inout")
    wk = g.ws(nws, "ws")
    rc = lib.sf_vsample(eng.handle, xio.ptr, arr, es.ptr, B, L0, steps, scale, int(use_graph), wk.ptr, nws, _l.stream_ptr(cuda))
    assert rc == 0, lib.sf_last_error().decode()
    g.verify_all()
    assert bool(torch.isfinite(xio.payload).all())
    assert torch.equal(_bytes(xio.payload), _bytes(plain))


def test_encoder_engine_forward(cuda):
    _l, lib = _lib()
    enc = small_encoder_module().to(cuda)
    B, L0 = 3, 1001
    y = torch.zeros(B, 1, L0)
    y[0, 0, 37] = y[1, 0, 1000] = y[2, 0, 0] = 1.0
    plain = enc._forward_engine(y.to(cuda), True)[1]["xs"][1:-1]
    torch.cuda.synchronize()
    eng = enc._engine
    nws = int(lib.sf_encoder1d_workspace_bytes(eng.handle, B, L0))
    assert nws > 0
    g = _G(cuda)
    ys = g.inp(y, "y")
    outs = [g.out(tuple(t.shape), torch.float32, f"xs{i}") for i, t in enumerate(plain)]
    arr = (ct.c_void_p * len(outs))(*[o.ptr for o in outs])
    wk = g.ws(nws, "ws")
    rc = lib.sf_encoder1d_forward(eng.handle, ys.ptr, B, L0, arr, wk.ptr, nws, _l.stream_ptr(cuda))
    assert rc == 0, lib.sf_last_error().decode()
    g.verify_all()
    assert len(outs) == len(SMALL_ENCODER["factors"]) + 1
    for o, p in zip(outs, plain):
        assert bool(torch.isfinite(o.payload).all()), o.name
        assert torch.equal(_bytes(o.payload), _bytes(p)), o.name


@pytest.fixture(scope="module")
def onset_nets(cuda):
    from syncfusion_amd.onset_net import VideoOnsetNet

    nets = {}
    for dt in ("fp32", "bf16"):
        net = VideoOnsetNet(False, dtype=dt)
        net.load_state_dict(seeded_state(net, 7))
        nets[dt] = net.to(cuda).eval()
    return nets


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 3, 45, 71), (1, 1, 7, 7)], ids=["2x3x45x71", "1x1x7x7"])
def test_onset_engine_forward(cuda, onset_nets, dtype, shape):
    _l, lib = _lib()
    N, T, H, W = shape
    net = onset_nets[dtype]
    x = torch.randn(N, 3, T, H, W, generator=torch.Generator().manual_seed(8))
    plain = net(x.to(cuda))
    torch.cuda.synchronize()
    eng = net._get_engine()
    nws = int(lib.sf_onsetnet_workspace_bytes(eng.handle, N, T, H, W))
    assert nws > 0
    g = _G(cuda)
    xs = g.inp(x, "frames")
    out = g.out((N, T), torch.float32, "logits")
    wk = g.ws(nws, "ws")
    rc = lib.sf_onsetnet_forward(eng.handle, xs.ptr, N, T, H, W, out.ptr, wk.ptr, nws, _l.stream_ptr(cuda))
    assert rc == 0, lib.sf_last_error().decode()
    g.verify_all()
    assert bool(torch.isfinite(out.payload).all())
    assert torch.equal(_bytes(out.payload), _bytes(plain))
