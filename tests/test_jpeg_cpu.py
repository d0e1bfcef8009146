"""JPEG decoder, host side (no GPU): the numpy reference against Pillow, ``parse_jpeg`` through the library against the reference parser,
and the shared reader / block decoder (syncfusion_amd/csrc/jpeg_decode.h) built for the host under ASan + UBSan."""
import io

import numpy as np
import pytest

import jpeg_host
import jpeg_ref as R


def test_reference_equals_pillow_small_grid():
    """Every combination of the axes on the small sizes: the reference's RGB equals Pillow's, byte for byte."""
    n = 0
    for H, W in R.SMALL_SIZES:
        for name, data in R.full_grid(H, W):
            _, rgb = R.decode(data)
            assert np.array_equal(rgb, R.pil_rgb(data)), name
            n += 1
    assert n == 5 * 4 * 4 * 2 * 2 * 4


@pytest.mark.parametrize("kind,sub,q,opt,rst", [("smooth", 2, 75, False, 0), ("noise", 1, 30, True, 2)])
def test_reference_equals_pillow_240x320(kind, sub, q, opt, rst):
    data = R.encode(R.content(kind, 240, 320, 5), q, sub, opt, rst)
    _, rgb = R.decode(data)
    assert np.array_equal(rgb, R.pil_rgb(data))


def test_reference_equals_pillow_16bit_tables():
    data = R.widen_dqt(R.encode(R.content("smooth", 29, 37), 90, 1))
    _, rgb = R.decode(data)
    assert np.array_equal(rgb, R.pil_rgb(data))


def _assert_info_equals_reference(info, ref):
    assert info.supported and ref["unsupported"] is None, (info.reason, ref["unsupported"])
    assert (info.width, info.height, info.components) == (ref["width"], ref["height"], ref["components"])
    assert info.sampling == ref["sampling"] and info.quant_selectors == ref["tq"]
    assert info.dc_selectors == ref["td"] and info.ac_selectors == ref["ta"]
    assert info.restart_interval == ref["restart_interval"] and info.mcus == ref["mcus"]
    assert info.data_range == ref["data_range"]
    assert info.segments == ref["segments"]
    assert set(info.quant_tables) == set(ref["quant"])
    for k, q in ref["quant"].items():
        assert np.array_equal(info.quant_tables[k], q) and info.quant_precision[k] == ref["quant_precision"][k]
    assert set(info.huffman_tables) == set(ref["huff"])
    for k, (counts, values) in ref["huff"].items():
        assert np.array_equal(info.huffman_tables[k][0], counts) and np.array_equal(info.huffman_tables[k][1], values)


def test_parse_jpeg_equals_reference_parser():
    from syncfusion_amd import parse_jpeg

    streams = R.small_grid() + [("240x320", R.encode(R.content("smooth", 240, 320), 75, 2, False, 4))]
    for name, data in streams:
        try:
            _assert_info_equals_reference(parse_jpeg(data), R.parse(data))
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e
    data = R.widen_dqt(R.encode(R.content("noise", 17, 33), 50, 2))        # 16-bit quantisation tables with values above 255
    info = parse_jpeg(data)
    assert set(info.quant_precision.values()) == {16} and max(int(q.max()) for q in info.quant_tables.values()) > 255
    _assert_info_equals_reference(info, R.parse(data))


def _sof_patched(data: bytes, luma_hv: int) -> bytes:
    k = data.find(b"\xff\xc0")
    assert k > 0 and data[k + 9] == 3
    b = bytearray(data)
    b[k + 11] = luma_hv
    return bytes(b)


def test_parse_jpeg_reports_unsupported_streams_with_reasons():
    from PIL import Image

    from syncfusion_amd import parse_jpeg

    arr = R.content("smooth", 17, 33)
    cases = {"progressive": R.encode(arr, 75, 2, progressive=True)}
    buf = io.BytesIO()
    Image.fromarray(arr).convert("CMYK").save(buf, "JPEG")
    cases["4 components"] = buf.getvalue()
    cases["sampling 1x2"] = _sof_patched(R.encode(arr, 75, 1), 0x12)     # h1v2 in the frame header of a 4:2:2 file
    try:
        rgb = R.encode(arr, 75, 0, keep_rgb=True)
    except (TypeError, ValueError, OSError):
        rgb = None
    if rgb is not None and rgb[rgb.find(b"\xff\xc0") + 10] == ord("R"):
        cases["R G B"] = rgb
    else:                                                                # the same thing by hand: ids R, G, B in frame and scan header
        b = bytearray(R.encode(arr, 75, 0))
        k, s = b.find(b"\xff\xc0"), b.find(b"\xff\xda")
        for i, ch in enumerate(b"RGB"):
            b[k + 10 + 3 * i] = ch
            b[s + 5 + 2 * i] = ch
        cases["R G B"] = bytes(b)
    for what, data in cases.items():
        info = parse_jpeg(data)
        assert not info.supported, what
        assert what in info.reason, (what, info.reason)
        assert (info.height, info.width) == (17, 33), what


def test_parse_jpeg_truncated_header_is_a_clean_error():
    from syncfusion_amd import parse_jpeg
    from syncfusion_amd._lib import SyncFusionAmdError

    data = R.encode(R.content("smooth", 17, 33), 75, 2, True, 2)
    header = R.parse(data)["data_range"][0]
    with pytest.raises(SyncFusionAmdError, match="malformed"):
        parse_jpeg(data[:20])
    with pytest.raises(SyncFusionAmdError):
        parse_jpeg(b"")
    with pytest.raises(SyncFusionAmdError):
        parse_jpeg(b"not a jpeg at all")
    for n in range(header):                       # every cut inside the header: an error with a message, never a crash
        with pytest.raises(SyncFusionAmdError, match="file 0 is malformed: .+"):
            parse_jpeg(data[:n])
    info = parse_jpeg(data[:header + 5])          # a cut inside the entropy-coded data is the decoder's to flag, not the parser's
    assert info.supported and info.data_range == (header, header + 5)


@pytest.fixture(scope="module")
def host_decoder(tmp_path_factory):
    d = tmp_path_factory.mktemp("jpeg_host")
    return jpeg_host.build(d), d


def test_host_build_of_shared_decoder_matches_reference(host_decoder):
    exe, d = host_decoder
    streams = R.small_grid() + [("240x320", R.encode(R.content("noise", 240, 320, 9), 75, 2, True, 3))]
    got = jpeg_host.run(exe, d, [s for _, s in streams], "ok")
    for (name, data), (status, checksum) in zip(streams, got):
        assert status == "ok", (name, status)
        assert checksum == R.coefficient_checksum(R.decode_coefficients(data)), name


def test_host_build_survives_corrupted_streams(host_decoder):
    """Truncation at every 7th byte and byte flips from a fixed LCG, on three small streams, under ASan + UBSan: every run ends with exit
    status 0 and no sanitizer report (jpeg_host.run asserts both), whether a status word is set or not."""
    exe, d = host_decoder
    seen = set()
    for i, data in enumerate(jpeg_host.corruption_streams()):
        blobs = jpeg_host.truncations(data) + jpeg_host.byte_flips(data, 300, 1234 + i)
        for status, _ in jpeg_host.run(exe, d, blobs, f"bad{i}_"):
            seen.add(status.split(":")[0])
    assert {"malformed", "flagged", "ok"} <= seen, seen      # the corruptions reach the parser, the decoder and harmless bytes alike


def test_host_build_flags_the_device_corruption_batch_as_the_reference_says(host_decoder):
    """The fixed batch the device corruption tests use goes through the sanitizer build here, and the status restatement of jpeg_ref
    (what those tests compare the device's status word with) is held equal to the shared decoder's over plain byte flips."""
    exe, d = host_decoder
    blobs, code = jpeg_host.device_corruption_batch()
    got = jpeg_host.run(exe, d, blobs, "dev")
    assert [st for st, _ in got] == ["ok", f"flagged:{R.ST_OUT_OF_BITS}", "ok", f"flagged:{code}"] and code != 0
    assert R.entropy_status(blobs[0]) == 0 and R.entropy_status(blobs[2]) == 0
    seen = set()
    for i, data in enumerate([blobs[2], R.encode(R.content("noise", 29, 37, 4), 30, 1, True, 0), R.encode(R.content("checker", 8, 8, 3), 95, 0, gray=True)]):
        flips = jpeg_host.plain_flips(data, 120, 40 + i)
        for f, (st, _) in zip(flips, jpeg_host.run(exe, d, flips, f"pf{i}_")):
            want = R.entropy_status(f)
            assert st == (f"flagged:{want}" if want else "ok"), (i, st, want)
            seen.add(want)
    assert {0, R.ST_OUT_OF_BITS} <= seen and len(seen) >= 3, seen
