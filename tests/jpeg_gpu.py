"""The raw device call of the JPEG tests: ``sf_jpeg_decode`` on buffers the test owns (optionally behind guard bands), so that the
coefficient workspace can be read back.  Plain module (not a conftest)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch


def raw_decode(blobs, device, guards=None):
    """Returns (out (N, H, W, 3) uint8 tensor, status (N,) int32 tensor, per-file coefficient planes or None, descriptors).
    With ``guards`` (guards.Guards) every device buffer is a guarded tensor: the file bytes, the descriptor and segment tables (inputs),
    the workspace (exactly sf_jpeg_decode_workspace_bytes), the status words and the output."""
    from syncfusion_amd import _lib, jpeg

    lib = _lib.load()
    st = jpeg._Staged([bytes(b) for b in blobs], pin=True)
    desc = st.desc
    ok = [i for i in range(st.n) if desc[i].status == jpeg.JPEG_OK]
    H, W = desc[ok[0]].height, desc[ok[0]].width
    ws_bytes = int(lib.sf_jpeg_decode_workspace_bytes(C.addressof(desc), st.n))
    assert ws_bytes >= 0
    nd, ns = st.n * C.sizeof(_lib.JpegDesc), st.n_segs * C.sizeof(_lib.JpegSegment)
    parts = [st.host[: st.n_bytes], st.host[st.desc_at: st.desc_at + nd], st.host[st.seg_at: st.seg_at + ns]]
    if guards is not None:
        dev = [guards.inp(p.to(device), name=n) for p, n in zip(parts, ("bytes", "descriptors", "segments"))]
        ws, status, out = guards.ws(ws_bytes, name="workspace"), guards.out((st.n,), torch.int32, name="status"), guards.out((st.n, H, W, 3), torch.uint8, name="out")
        ptr = lambda t: t.data_ptr()
        view = lambda t: t.payload
    else:
        dev = [p.to(device) for p in parts]
        ws, status, out = (torch.empty(max(16, ws_bytes), dtype=torch.uint8, device=device), torch.empty(st.n, dtype=torch.int32, device=device),
                           torch.empty((st.n, H, W, 3), dtype=torch.uint8, device=device))
        ptr = lambda t: t.data_ptr()
        view = lambda t: t
    ws.payload.fill_(0xFF) if guards is not None else ws.fill_(0xFF)      # the call relies on nothing the caller left there
    _lib.check(lib.sf_jpeg_decode(ptr(dev[0]), st.n_bytes, C.addressof(desc), ptr(dev[1]), ptr(dev[2]), st.n_segs, st.n, H, W, ptr(out), ptr(status),
                                  ptr(ws), ws_bytes, _lib.stream_ptr(device)), "sf_jpeg_decode")
    torch.cuda.synchronize(device)
    raw = view(ws).cpu().numpy()
    coefs = []
    for i in range(st.n):
        d = desc[i]
        if d.status != jpeg.JPEG_OK:
            coefs.append(None)
            continue
        planes, at = [], d.coef_offset * 2
        for c in range(d.ncomp):
            bh, bw = d.mcus_y * d.v[c], d.mcus_x * d.h[c]
            planes.append(raw[at: at + bh * bw * 128].view(np.int16).reshape(bh, bw, 64).copy())
            at += bh * bw * 128
        coefs.append(planes)
    return view(out), view(status), coefs, desc
