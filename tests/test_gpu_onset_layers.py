"""Every convolution of the VideoOnsetNet inference engine, element-wise against fp64 (GPU).

The engine's detail taps (sf_onsetnet_debug_detail) give the output of each of the 37 launch sequences; tests/onset_layers_ref.py
recomputes each one in fp64 from the device's own tap of its input and holds EVERY element to the derived bound
|dev - ref| <= u |ref| + c (K + 3) 2^-24 A (no tolerance here is fitted to a device measurement).  The 16-bit runs are asserted to have
gone through the three special kernels (conv_sp.hip, conv_tw.hip, onset_stem.hip) and the two-launch column split, which the fp32
gates never reach.  The stage-level tests of test_gpu_models.py stay as they are.
"""
import time

import pytest
import torch

import onset_layers_ref as R
from helpers import seeded_state

pytestmark = pytest.mark.gpu

EDGE_SHAPES = [(1, 1, 32, 32), (2, 2, 24, 40), (1, 3, 36, 60), (3, 7, 48, 32), (2, 5, 20, 116)]     # test_onsetnet_edge_shapes'
ODD_SHAPES = [(1, 2, 29, 35), (2, 3, 45, 71), (1, 1, 7, 7), (2, 4, 113, 111)]   # odd extents at the stride-2 stem and layer 2-4 entries
REAL_SHAPES = [(2, 4, 112, 112)]
CKPT_SHAPES = [(2, 3, 45, 71), (2, 4, 112, 112)]
CKPT_SEED = 11          # chosen on the CPU (test_onset_layers_cpu.py checks the range on these shapes)
FP16_RANGE = 65504.0 / 4
MAX_TAP_FLOATS = 1 << 30
STAGE_OF = {"stem": "stem.3", "layer1": "layer1.1.conv2.0.3", "layer2": "layer2.1.conv2.0.3", "layer3": "layer3.1.conv2.0.3",
            "layer4": "layer4.1.conv2.0.3"}


def pad_to(x, m):
    return (x + m - 1) // m * m


def tw_ok(cin: int, cin_ld: int, cout: int) -> bool:
    """conv_tw_ok for a 16-bit type: 64 outputs, 4 or 10 sixteen-channel K steps that lie inside the input rows."""
    ks = 4 if cin <= 64 else (10 if cin <= 160 else 0)
    return cout == 64 and ks > 0 and 16 * ks <= cin_ld and cin_ld % 8 == 0


def sp_ok(cin: int, cin_ld: int, cout: int, cout_ld: int) -> bool:
    """conv_sp_ok for a 16-bit type: 64 input channels in 64-channel rows, output rows of exactly ceil(cout / 32) <= 8 column tiles."""
    ntiles = (cout + 31) // 32
    return cin == 64 and cin_ld == 64 and cout_ld == 32 * ntiles and ntiles <= 8


PLANES = {"layer1": 64, "layer2": 128, "layer3": 256, "layer4": 512}


def expected_path(layer: R.Layer, dtype: str) -> str:
    """The launch sequence the engine picks, restated from its own conditions (onset_engine.cpp sf_onsetnet_create / make_conv /
    OnsetExec::conv): the special kernels and the column split are 16-bit only."""
    if dtype == "fp32":
        return "conv_gemm"
    if layer.name == "stem.0":
        return "onset_stem"                          # RGB rows of 4, 45 outputs in rows of 64 (and < 2^31 input bytes: every shape here)
    if layer.name == "stem.3":
        cin_ld, cout_ld = 64, 64
    else:
        # a block's mid tensor travels in rows padded to 32 where its temporal convolution runs as the frame walk, else to 64
        planes = PLANES[layer.name.split(".")[0]]
        mid = layer.cin if layer.kernel == (3, 1, 1) else layer.cout
        mid_ld = pad_to(mid, 32) if tw_ok(mid, pad_to(mid, 32), planes) else pad_to(mid, 64)
        cin_ld = mid_ld if layer.kernel == (3, 1, 1) else pad_to(layer.cin, 64)
        cout_ld = mid_ld if layer.kernel == (1, 3, 3) else pad_to(layer.cout, 64)
    if layer.kernel == (1, 3, 3) and layer.stride == 1 and sp_ok(layer.cin, cin_ld, layer.cout, cout_ld):
        return "conv_sp"
    if layer.kernel == (3, 1, 1) and tw_ok(layer.cin, cin_ld, layer.cout):
        return "conv_tw"
    q192 = layer.cout // 192                         # whole 192-wide tiles, then the remaining <= 128 columns as a second launch
    rest = cout_ld - 192 * q192
    cols_now = min(pad_to(cout_ld, 128), pad_to(cout_ld, 192))
    if q192 >= 1 and 0 < rest <= 128 and layer.cout > 192 * q192 and 192 * q192 + 128 < cols_now:
        return "conv_gemm_split"
    return "conv_gemm"


def tap_floats(shape, n_sel: int) -> int:
    """fp32 elements of the 37 convolution taps + 5 stage taps of one forward with n_sel clips copied."""
    _, t, h, w = shape
    hw, total, per = {"input": (h, w)}, 0, {}
    for layer in R.onset_layers():
        hw[layer.name] = R.out_hw(*hw[layer.src], layer)
        per[layer.name] = n_sel * t * hw[layer.name][0] * hw[layer.name][1] * layer.cout
        total += per[layer.name]
    return total + sum(per[v] for v in STAGE_OF.values())


def run_case(cuda, shape, dtype, state, x, clips=None, max_abs=None):
    from syncfusion_amd.onset_net import VideoOnsetNet

    n, t, h, w = shape
    net = VideoOnsetNet(pretrained=False, dtype=dtype)
    net.load_state_dict(state)
    net = net.to(cuda).eval()
    gx = x.to(cuda)
    y_plain = net(gx)                                   # the untapped production call
    cap = tap_floats(shape, len(clips) if clips is not None else n)
    assert cap <= MAX_TAP_FLOATS, cap
    taps, paths = {}, {}
    y = net._get_engine().forward(gx, taps, cap_floats=cap, detail=True, clips=clips, paths=paths)   # the buffer is exactly as large as needed
    assert torch.equal(y, y_plain), "logits with the detail taps on differ from the untapped call"
    layers = R.onset_layers()
    assert len(layers) == 37 and set(taps) == {l_.name for l_ in layers} | set(STAGE_OF), sorted(taps)
    for stage, conv in STAGE_OF.items():                # the stage taps keep their names and are the block outputs
        assert torch.equal(taps[stage], taps[conv]), stage
    # which kernels ran: a 16-bit run that fell back to conv_gemm would prove nothing about conv_sp / conv_tw / onset_stem
    want = {l_.name: expected_path(l_, dtype) for l_ in layers}
    got = {k: v for k, v in paths.items() if k in want}
    assert got == want, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}
    if dtype != "fp32":
        by = lambda p: sorted(k for k, v in got.items() if v == p)   # noqa: E731
        assert by("conv_sp") == sorted(f"layer1.{b}.conv{c}.0.0" for b in (0, 1) for c in (1, 2))          # cin_ld == 64 spatial convolutions
        assert by("conv_tw") == sorted(["stem.3"] + [f"layer1.{b}.conv{c}.0.3" for b in (0, 1) for c in (1, 2)])   # 64-output temporal ones
        assert by("onset_stem") == ["stem.0"] and by("conv_gemm_split") == ["layer2.1.conv1.0.0", "layer2.1.conv2.0.0"]
    tag = f"onset layers {shape} {dtype}" + (f" clips {list(clips)}" if clips is not None else "")
    res = R.check_all_layers(state, x, {k: v.cpu() for k, v in taps.items()}, dtype, tag, clips, paths, max_abs)
    worst = max(res, key=lambda k: res[k][0])
    print(f"{tag}: worst err/bound {res[worst][0]:.3f} at {worst} ({paths[worst]})")
    return res


def _case(shape, seed_w, seed_x):
    from syncfusion_amd.onset_net import VideoOnsetNet

    n, t, h, w = shape
    state = seeded_state(VideoOnsetNet(pretrained=False), seed_w)
    x = torch.randn(n, 3, t, h, w, generator=torch.Generator().manual_seed(seed_x))
    return state, x


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", EDGE_SHAPES + ODD_SHAPES + REAL_SHAPES)
def test_onset_every_convolution_against_fp64(cuda, shape, dtype):
    """37 taps per case, every element inside the derived bound: the five even edge shapes of the stage-level test, odd heights and
    widths (the stride-2 stem and the stride-2 first blocks of layers 2-4 see odd extents; (1, 1, 7, 7) is the smallest shape the
    engine accepts) and the real 112 x 112 frame."""
    n, t, h, w = shape
    state, x = _case(shape, 4242 + t, 17 * h + w)
    run_case(cuda, shape, dtype, state, x)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", CKPT_SHAPES)
def test_onset_every_convolution_checkpoint_like_weights(cuda, shape, dtype):
    """Running variances over five decades, means up to +-3 and four exactly-zero folded channels per BatchNorm
    (onset_layers_ref.checkpoint_like_state): large shifts cancelling against the convolution, and relu(shift) where the folded weight
    is zero.  The fp64 reference first shows that no activation leaves a quarter of the fp16 range, so a failure is a kernel's."""
    from syncfusion_amd.onset_net import VideoOnsetNet

    n, t, h, w = shape
    state = R.checkpoint_like_state(VideoOnsetNet(pretrained=False), CKPT_SEED)
    x = torch.randn(n, 3, t, h, w, generator=torch.Generator().manual_seed(17 * h + w + 1))
    run_case(cuda, shape, dtype, state, x, max_abs=FP16_RANGE)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_onset_every_convolution_benchmarked_shape_n32(cuda, dtype):
    """The benchmarked 32 x (3, 30, 112, 112) forward (the macro tiles of conv_gemm_mt.hip, the 32-clip grids of conv_sp / conv_tw) with
    the detail taps restricted to clips 0 and 31, the clips test_onsetnet_benchmarked_shape_n32 checks: 3.2e8 floats of tap buffer.
    The fp64 reference of the two clips -- ref and A of all 37 convolutions, EVERY element (no subset), plus the gate -- is 1.2 TFLOP
    and was timed at 20 s on 8 host threads; a whole case (engine build, two 32-clip forwards, copies, reference, gate) was measured at
    15.8 s (fp32), 17.0 s (bf16) and 19.5 s (fp16) beside an MI355X with 16 host threads.  Timeout = 3 x the slowest."""
    state, x = _case((32, 30, 112, 112), 4000, 4000)      # test_gpu_models._onset_n32_case's weights and input
    t0 = time.time()
    run_case(cuda, (32, 30, 112, 112), dtype, state, x, clips=[0, 31])
    print(f"onset layers N=32 {dtype}: {time.time() - t0:.1f} s")
