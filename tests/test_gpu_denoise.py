"""GPU suite of the STFT pair and the spectral-gating denoiser (syncfusion_amd/csrc/stft.hip through sf_stft_forward, sf_istft_forward,
sf_spectral_gate_noise_threshold and sf_spectral_gate) against the fp64 restatement in tests/denoise_ref.py, which
tests/test_denoise_cpu.py pins to scipy.signal.

Shapes (denoise_ref.SHAPES, sr 48000): the smallest at which each mechanism can go wrong -- more smoothing taps than frames, a hop that does
not divide the window, L = window, a tail behind the last frame, a multiple of the hop, every frame holding padding -- and one chunked call
(chunk_size 4096, padding 512, L = 10000, 2 channels).  B = 5 (row 1 all zero, row 2 scaled by 1e-4) and B = 1.  Every call goes through
the C ABI with guard bands around every buffer (tests/guards.py) and a workspace of exactly the queried size.

Figures (denoise_ref.errors): spectra and waveforms as the largest absolute error over the row's largest reference magnitude, masks as the
largest absolute error.  Gates are 10 x the error of the same stages in plain fp32 on the host (denoise_ref.gate_f32: torch's fp32 FFT,
numpy float32 loops) against fp64 on these very inputs, `python tests/denoise_ref.py`:

    figure                    fp32 floor   gate       largest on an MI355X
    STFT bins                 1.35e-07     1.35e-06   1.71e-07
    istft(stft(x)) - x        2.88e-07     2.88e-06   2.66e-07
    unsmoothed mask           3.51e-05     3.51e-04   6.20e-05
    smoothed mask             1.75e-06     1.75e-05   1.81e-06
    output                    4.25e-07     4.25e-06   3.89e-07
    stationary smoothed mask  8.01e-08     8.01e-07   6.34e-08
    stationary output         6.31e-08     6.31e-07   1.92e-07 (the chunked call; 6.01e-08 on whole rows)

(the unsmoothed mask is a sigmoid of slope 10 on (|S| - sm) / sm: bins far below the plane's maximum carry fp32's absolute rounding of the
transform as a large relative error).  Stationary mode: the device's binary mask must equal the restatement's in every cell whose dB lies
at least 1e-2 dB from its threshold; at most 0.2 % of the cells of the non-zero rows may be left out by that rule (largest here: 0.071 %,
counted on the restatement's own dB planes).  In the all-zero row every cell sits ON its threshold (a constant plane): there the mask must
be 0 in every cell instead.  The stationary output is compared with the restatement fed the DEVICE's binary mask, so a flipped cell cannot hide an error
further downstream.
"""
import functools

import numpy as np
import pytest
import torch

import denoise_ref as R
from guards import Guards

pytestmark = pytest.mark.gpu

NB = 5
GATES = {"spec": 1.35e-6, "roundtrip": 2.88e-6, "mask_raw": 3.51e-4, "mask_smooth": 1.75e-5, "out": 4.25e-6,
         "stationary_mask_smooth": 8.01e-7, "stationary_out": 6.31e-7}
MARGIN_DB, LEFT_OUT = 1e-2, 2e-3
ST_PROP = 0.9
IDS = [f"{n}-{h}-{L}" for n, h, L in R.SHAPES]


@functools.lru_cache(maxsize=None)
def inputs(L):
    return R.make_rows(L, NB)


@functools.lru_cache(maxsize=None)
def reference(n_fft, hop, L):
    """fp64 results of the non-stationary path and the stationary thresholds / dB planes for the NB rows.  Computed once, never modified."""
    out = []
    for x in inputs(L):
        r = R.gate_ref(x, R.SR, n_fft, hop)
        r["thresh"] = R.stationary_threshold(r["spec"])
        r["db"] = R.amp_db(r["spec"])
        out.append(r)
    return out


def plan_for(n_fft, hop, device, **kw):
    from syncfusion_amd import denoise

    vf, vt = denoise.smoothing_taps(R.SR, n_fft, hop, 500.0, 50.0)
    return denoise._plan(device, n_fft, hop, kw.pop("win", n_fft), kw.pop("center", True), kw.pop("pad_mode", "constant"),
                         kw.pop("scaling", "spectrum"), vf, vt)


def planes(t):
    """(B, T, F[, 2]) device payload -> (B, F, T) numpy, complex128 for a spectrum"""
    a = t.cpu().numpy().astype(np.float64)
    if a.ndim == 4:
        a = a[..., 0] + 1j * a[..., 1]
    return np.ascontiguousarray(a.transpose(0, 2, 1))


def run_gate(plan, rows, b=None, prop=1.0, thresh=None, prop_first=None, device="cuda:0"):
    """sf_spectral_gate on (B, L) host rows with every buffer guarded; -> dict of numpy results, (B, F, T) planes"""
    from syncfusion_amd import _lib, denoise

    lib = _lib.load()
    dev = torch.device(device)
    B, L = rows.shape
    T, F = plan.frames(L), plan.bins
    assert lib.sf_spectral_gate_frames(plan.handle, L) == T
    need = plan.workspace_bytes(B, L)
    assert need > 0
    g = Guards(dev)
    x = g.inp(torch.tensor(rows), "wav")
    th = g.inp(torch.from_numpy(np.ascontiguousarray(thresh, dtype=np.float32)), "thresh") if thresh is not None else None
    spec, m0, m1 = g.out((B, T, F, 2), name="spec", ld=2 * F), g.out((B, T, F), name="mask_raw"), g.out((B, T, F), name="mask_smooth")
    out, ws = g.out((B, L), name="out"), g.ws(need, "ws")
    b = denoise.smoothing_coefficient(2.0, R.SR, plan.hop) if b is None else b
    with torch.cuda.device(dev):
        _lib.check(lib.sf_spectral_gate(plan.handle, x.data_ptr(), B, L, int(thresh is not None), float(b), 2.0, 10.0, float(prop),
                                        int(thresh is not None if prop_first is None else prop_first), th.data_ptr() if th is not None else None, spec.data_ptr(), m0.data_ptr(), m1.data_ptr(), out.data_ptr(),
                                        ws.data_ptr(), need, _lib.stream_ptr(dev)), "sf_spectral_gate")
    g.verify_all()
    res = {"spec": planes(spec.payload), "mask_raw": planes(m0.payload), "mask_smooth": planes(m1.payload), "out": out.payload.cpu().numpy(),
           "raw_bits": (spec.payload.clone(), m0.payload.clone(), m1.payload.clone(), out.payload.clone())}
    for k in ("spec", "mask_raw", "mask_smooth", "out"):
        assert np.isfinite(res[k]).all(), f"{k}: a cell was not written or is not finite"
    return res


def run_stft_istft(plan, rows, device="cuda:0"):
    """sf_stft_forward, then sf_istft_forward back to L samples, guarded; -> ((B, F, T) complex128, (B, L) float32, device spectrum)"""
    from syncfusion_amd import _lib

    lib = _lib.load()
    dev = torch.device(device)
    B, L = rows.shape
    T, F = plan.frames(L), plan.bins
    g = Guards(dev)
    x = g.inp(torch.tensor(rows), "wav")
    spec = g.out((B, T, F, 2), name="spec", ld=2 * F)
    with torch.cuda.device(dev):
        _lib.check(lib.sf_stft_forward(plan.handle, x.data_ptr(), B, L, spec.data_ptr(), _lib.stream_ptr(dev)), "sf_stft_forward")
    g.verify_all()
    S = spec.payload.clone()
    need = plan.workspace_bytes(B, plan.samples(T))
    g2 = Guards(dev)
    s_in, y, ws = g2.inp(S, "spec", ld=2 * F), g2.out((B, L), name="wave"), g2.ws(need, "ws")
    with torch.cuda.device(dev):
        _lib.check(lib.sf_istft_forward(plan.handle, s_in.data_ptr(), B, T, y.data_ptr(), L, ws.data_ptr(), need, _lib.stream_ptr(dev)), "sf_istft_forward")
    g2.verify_all()
    return planes(S), y.payload.cpu().numpy(), S


def row_errors(res, i, ref, x, hop):
    return R.errors({k: res[k][i] for k in ("spec", "mask_raw", "mask_smooth", "out")}, ref, x, hop)


def check(errs, prefix=""):
    print({k: f"{v:.3e}" for k, v in errs.items()})
    for k, v in errs.items():
        gate = GATES.get(prefix + k, GATES.get(k))
        assert v <= gate, f"{prefix}{k}: {v:.3e} above the gate {gate:.3e}"


@pytest.mark.parametrize("n_fft,hop,L", R.SHAPES, ids=IDS)
def test_stft_bins_and_round_trip(n_fft, hop, L):
    rows, refs = inputs(L), reference(n_fft, hop, L)
    plan = plan_for(n_fft, hop, "cuda:0")
    S, y, _ = run_stft_istft(plan, rows)
    n = (plan.frames(L) - 1) * hop
    worst = {"spec": 0.0, "roundtrip": 0.0}
    for i in range(NB):
        if not rows[i].any():
            assert not S[i].any() and not y[i].any()
            continue
        worst["spec"] = max(worst["spec"], float(np.abs(S[i] - refs[i]["spec"]).max() / np.abs(refs[i]["spec"]).max()))
        worst["roundtrip"] = max(worst["roundtrip"], float(np.abs(y[i, :n].astype(np.float64) - rows[i, :n]).max() / np.abs(rows[i]).max()))
        assert not y[i, n:].any()                        # the tail behind the last frame stays zero
    check(worst)
    S1, y1, _ = run_stft_istft(plan, rows[3:4])             # alone and inside the batch: the same bits
    assert np.array_equal(S1[0], S[3]) and np.array_equal(y1[0], y[3])


@pytest.mark.parametrize("n_fft,hop,L", R.SHAPES, ids=IDS)
def test_nonstationary_gate(n_fft, hop, L):
    rows, refs = inputs(L), reference(n_fft, hop, L)
    plan = plan_for(n_fft, hop, "cuda:0")
    res = run_gate(plan, rows)
    worst = {}
    for i in range(NB):
        if not rows[i].any():                              # the documented deviation: mask 0, output 0
            assert not res["spec"][i].any() and not res["mask_raw"][i].any() and not res["out"][i].any()
            continue
        for k, v in row_errors(res, i, refs[i], rows[i], hop).items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert not res["out"][i, (plan.frames(L) - 1) * hop:].any()
    check(worst)
    for i in (1, 3):                                        # a row's result is bit-equal alone and inside the batch
        alone = run_gate(plan, rows[i:i + 1])
        for a, b in zip(alone["raw_bits"], res["raw_bits"]):
            assert torch.equal(a[0], b[i])
    # prop_decrease < 1 is applied AFTER the smoothing here
    part = run_gate(plan, rows[0:1], prop=0.8)
    check(row_errors(part, 0, R.gate_ref(rows[0], R.SR, n_fft, hop, prop_decrease=0.8), rows[0], hop))
    swapped = run_gate(plan, rows[0:1], prop=0.8, prop_first=True)      # ... and BEFORE it on request: different at the plane's edges
    check(row_errors(swapped, 0, R.gate_ref(rows[0], R.SR, n_fft, hop, prop_decrease=0.8, prop_before_smoothing=True), rows[0], hop))
    assert np.abs(swapped["mask_smooth"] - part["mask_smooth"]).max() > 1e-3


@pytest.mark.parametrize("n_fft,hop,L", R.SHAPES, ids=IDS)
def test_stationary_gate(n_fft, hop, L):
    from syncfusion_amd import _lib

    rows, refs = inputs(L), reference(n_fft, hop, L)
    plan = plan_for(n_fft, hop, "cuda:0")
    lib, dev = _lib.load(), torch.device("cuda:0")
    F = plan.bins
    need = plan.workspace_bytes(NB, L)
    g = Guards(dev)
    x, th, ws = g.inp(torch.tensor(rows), "noise"), g.out((NB, F), name="thresh"), g.ws(need, "ws")
    with torch.cuda.device(dev):
        _lib.check(lib.sf_spectral_gate_noise_threshold(plan.handle, x.data_ptr(), NB, L, 1.5, th.data_ptr(), ws.data_ptr(), need,
                                                        _lib.stream_ptr(dev)), "sf_spectral_gate_noise_threshold")
    g.verify_all()
    thresh = th.payload.cpu().numpy()
    assert np.isfinite(thresh).all()
    res = run_gate(plan, rows, prop=ST_PROP, thresh=thresh)
    left_out = cells = 0
    worst = {}
    for i in range(NB):
        raw = res["mask_raw"][i]
        assert np.isin(raw, (0.0, 1.0)).all()
        if not rows[i].any():
            assert not raw.any() and not res["out"][i].any()
            continue
        want = refs[i]["db"] > refs[i]["thresh"][:, None]
        decided = np.abs(refs[i]["db"] - refs[i]["thresh"][:, None]) >= MARGIN_DB
        assert np.array_equal(raw[decided] > 0.5, want[decided]), f"row {i}: {int(((raw > 0.5) != want)[decided].sum())} decided cells differ"
        left_out += int((~decided).sum())
        cells += decided.size
        fed = R.gate_ref(rows[i], R.SR, n_fft, hop, stationary=True, prop_decrease=ST_PROP, mask_raw=raw)
        e = row_errors(res, i, fed, rows[i], hop)
        for k in ("spec", "mask_smooth", "out"):
            worst[k] = max(worst.get(k, 0.0), e[k])
    print(f"left out by the margin rule: {left_out} of {cells} cells ({left_out / cells:.3%})")
    assert left_out <= LEFT_OUT * cells
    check(worst, "stationary_")
    alone = run_gate(plan, rows[3:4], prop=ST_PROP, thresh=thresh[3:4])
    for a, b in zip(alone["raw_bits"], res["raw_bits"]):
        assert torch.equal(a[0], b[3])


@pytest.mark.parametrize("kw", [dict(pad_mode="reflect"), dict(center=False), dict(win_length=200), dict(scaling=None),
                                dict(win_length=200, center=False, scaling=None)], ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_python_stft_pair_options(kw):
    """the public stft / istft with every option away from the denoiser's: bins against fp64, and istft(stft(x)) against x"""
    from syncfusion_amd import istft, stft

    n_fft, hop, L = 256, 50, 3000
    x = inputs(L)[[0, 3]]
    dev = torch.device("cuda:0")
    win, center, scaling = kw.get("win_length"), kw.get("center", True), kw.get("scaling", "spectrum")
    S = stft(torch.from_numpy(x).to(dev), n_fft, hop, win_length=win, center=center, pad_mode=kw.get("pad_mode", "constant"), scaling=scaling)
    assert S.dtype == torch.complex64 and S.shape[:2] == (2, n_fft // 2 + 1)
    w = win or n_fft
    for i in range(2):
        ref = R.stft_ref(x[i], n_fft, hop, w, center, kw.get("pad_mode", "constant"), scaling)
        got = S[i].cpu().numpy().astype(np.complex128)
        assert got.shape == ref.shape
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        print(f"spec {err:.3e}")
        assert err <= GATES["spec"]
    if kw.get("pad_mode") == "reflect":
        return                                            # the inverse assumes nothing about the padding; reflect changes only the edges' bins
    y = istft(S, n_fft, hop, win_length=win, center=center, scaling=scaling, length=L)
    assert tuple(y.shape) == (2, L)
    n = w + (S.shape[-1] - 1) * hop - 2 * (w // 2 if center else 0)
    lo = 0 if center else w                                # uncentred: the first and last window are covered by vanishing window values
    y = y.cpu().numpy().astype(np.float64)
    err = float(np.abs(y[:, lo:n - lo] - x[:, lo:n - lo]).max() / np.abs(x).max())
    print(f"roundtrip {err:.3e}")
    assert err <= GATES["roundtrip"] and not y[:, n:].any()
    one = stft(torch.from_numpy(x[0]).to(dev), n_fft, hop, win_length=win, center=center, scaling=scaling)
    assert one.shape == S.shape[1:] and torch.equal(torch.view_as_real(one.contiguous()), torch.view_as_real(S[0].contiguous()))


def test_chunked_reduce_noise():
    """chunk_size 4096, padding 512, L = 10000, 2 channels: three padded chunks per channel, six rows in one device batch"""
    from syncfusion_amd import reduce_noise

    L, chunk, pad, n_fft, hop = 10000, 4096, 512, 1024, 256
    y = np.ascontiguousarray(inputs(L)[[0, 3]])
    ref = R.reduce_noise_ref(y, R.SR, n_fft=n_fft, hop=hop, chunk_size=chunk, padding=pad)
    out, parts = reduce_noise(y, R.SR, n_fft=n_fft, hop_length=hop, chunk_size=chunk, padding=pad, return_parts=True)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == y.shape
    T = (chunk + 2 * pad) // hop + 1
    assert tuple(parts["spec"].shape) == (6, T, n_fft // 2 + 1, 2) and tuple(parts["mask_raw"].shape) == tuple(parts["mask_smooth"].shape) == (6, T, n_fft // 2 + 1)
    assert len(parts["chunks"]) == 3 and tuple(parts["rows"].shape) == (6, chunk + 2 * pad)
    err = float((np.abs(out - ref).max(axis=1) / np.abs(y).max(axis=1)).max())
    print(f"out {err:.3e}")
    assert err <= GATES["out"]
    t = reduce_noise(torch.from_numpy(y[1]).to("cuda:0"), R.SR, n_fft=n_fft, hop_length=hop, chunk_size=chunk, padding=pad)   # (L,) device tensor
    assert isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == (L,) and np.array_equal(t.cpu().numpy(), out[1])
    # stationary: one threshold row per channel (from the channel's first chunk_size samples), shared by the channel's three chunks
    from syncfusion_amd import denoise

    s, sp = reduce_noise(y, R.SR, stationary=True, prop_decrease=ST_PROP, n_fft=n_fft, hop_length=hop, chunk_size=chunk, padding=pad, return_parts=True)
    rows = denoise.split_rows(y.astype(np.float64), parts["chunks"])
    raw = planes(sp["mask_raw"])
    fed, left_out = [], 0
    for r in range(6):
        th = R.stationary_threshold(R.stft_ref(y[r // 3, :chunk].astype(np.float64), n_fft, hop))
        db = R.amp_db(R.stft_ref(rows[r], n_fft, hop))
        decided = np.abs(db - th[:, None]) >= MARGIN_DB
        assert np.array_equal(raw[r][decided] > 0.5, (db > th[:, None])[decided]), f"row {r}"
        left_out += int((~decided).sum())
        fed.append(R.gate_ref(rows[r], R.SR, n_fft, hop, stationary=True, prop_decrease=ST_PROP, mask_raw=raw[r])["out"])
    assert left_out <= LEFT_OUT * raw.size
    ref_s = denoise.merge_rows(np.stack(fed), parts["chunks"], 2, L)
    err = float((np.abs(s - ref_s).max(axis=1) / np.abs(y).max(axis=1)).max())
    print(f"stationary out {err:.3e}, left out {left_out} of {raw.size}")
    assert s.shape == y.shape and err <= GATES["stationary_out"]
