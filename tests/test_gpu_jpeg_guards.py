"""Guard bands around every buffer of the device JPEG decode (tests/guards.py): the file bytes, the descriptor and segment tables, the
workspace of exactly ``sf_jpeg_decode_workspace_bytes``, the status words and the output -- for a well-formed batch and a corrupted one."""
from __future__ import annotations

import numpy as np
import pytest

import jpeg_host
import jpeg_ref as R
from guards import Guards
from jpeg_gpu import raw_decode

pytestmark = pytest.mark.gpu


def test_decode_stays_inside_its_buffers_17x33_420(cuda):
    blobs = [R.encode(R.content(k, 17, 33, i), q, 2, opt, rst) for i, (k, q, opt, rst) in
             enumerate((("smooth", 75, False, 0), ("noise", 30, True, 2), ("checker", 95, True, 0), ("saturated", 5, False, 1)))]
    with Guards(cuda) as g:
        out, status, _, _ = raw_decode(blobs, cuda, guards=g)
    assert status.cpu().tolist() == [0, 0, 0, 0]
    assert np.array_equal(out.cpu().numpy(), np.stack([R.pil_rgb(b) for b in blobs]))


def test_corrupted_batch_stays_inside_its_buffers(cuda):
    """The fixed corrupted batch (jpeg_host.device_corruption_batch; test_jpeg_cpu.py runs it through the host build under ASan + UBSan)
    plus more plain byte flips of its second stream."""
    blobs, code = jpeg_host.device_corruption_batch()
    extra = jpeg_host.plain_flips(blobs[2], 6, 7)
    batch = blobs + extra
    with Guards(cuda) as g:
        out, status, _, _ = raw_decode(batch, cuda, guards=g)
    assert status.cpu().tolist()[:4] == [0, status[1].item(), 0, code] and status[1].item() != 0
    assert status.cpu().tolist()[4:] == [R.entropy_status(f) for f in extra]
    got = out.cpu().numpy()
    assert np.array_equal(got[0], R.pil_rgb(blobs[0])) and np.array_equal(got[2], R.pil_rgb(blobs[2]))
