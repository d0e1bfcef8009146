"""The guard-band helper (tests/guards.py) on CPU tensors: verify() must fail for every kind of stray access the GPU tests rely on
it to see, and pass when only the payload was written.  Every write stays inside the helper's own allocation."""
import pytest
import torch

import guards
from guards import Guards, guard_bytes, guarded

CPU = torch.device("cpu")
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def test_guard_size_is_the_larger_of_64k_and_256_rows_rounded_to_pages():
    assert guard_bytes(1, 4) == 64 << 10
    assert guard_bytes(64, 4) == 64 << 10                    # 256 rows of 64 floats = exactly 64 KiB
    assert guard_bytes(65, 4) == 256 * 65 * 4 + 4096 - (256 * 65 * 4) % 4096
    assert guard_bytes(1024, 4) == 1 << 20
    assert guard_bytes(1023, 2) % 4096 == 0 and guard_bytes(1023, 2) >= 256 * 1023 * 2
    t = guarded((3, 7, 320), torch.float32, CPU, "out")
    assert t.guard == 256 * 320 * 4 and t.front_guard().numel() == t.tail_guard().numel() == t.guard


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(5,), (3, 37, 8), (2, 1, 33)])
def test_layout_alignment_and_fills(dtype, shape):
    t = guarded(shape, dtype, CPU, "out")
    assert t.ptr % 256 == 0 and t.payload.data_ptr() == t.ptr
    assert tuple(t.payload.shape) == shape and t.payload.dtype == dtype and t.payload.is_contiguous()
    # the tail guard starts at the very next byte after the last payload element
    assert t.end - t.start == t.payload.numel() * t.payload.element_size()
    assert t.tail_guard().data_ptr() == t.ptr + t.nbytes
    assert bool(torch.isnan(t.payload).all()), "an untouched output payload reads as NaN"
    assert bool((t.front_guard() == 0xA5).all()) and bool((t.tail_guard() == 0xA5).all())
    t.verify()


def test_input_and_workspace_fills():
    x = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    t = guarded(x.shape, x.dtype, CPU, "in", init=x)
    assert torch.equal(t.payload, x)
    assert bool((t.front_guard() == 0xFF).all()) and bool((t.tail_guard() == 0xFF).all())
    assert bool(torch.isnan(t.front_guard().view(torch.float32)).all())      # a read past an input picks up NaN
    t.verify()
    w = guarded(1001, torch.uint8, CPU, "ws")
    assert w.nbytes == 1001 and w.payload.numel() == 1001, "exactly the byte count asked for"
    assert bool((w.payload == 0xFF).all()) and bool((w.tail_guard() == 0xA5).all())
    w.verify()
    e = guarded(0, torch.uint8, CPU, "ws")                                   # an empty workspace still has an address and two guards
    assert e.nbytes == 0 and e.ptr % 256 == 0 and e.ptr != 0
    e.verify()
    with pytest.raises(ValueError):
        guarded((2,), torch.float32, CPU, "in")
    with pytest.raises(ValueError):
        guarded((2,), torch.float32, CPU, "nonsense")


@pytest.mark.parametrize("dtype", DTYPES)
def test_payload_writes_pass(dtype):
    t = guarded((4, 9), dtype, CPU, "out")
    t.payload.copy_(torch.randn(4, 9).to(dtype))
    t.verify()
    assert bool(torch.isfinite(t.payload).all())


def _elem_view(t, byte_offset_from_buf_start, dtype):
    """one element of `dtype` at a byte offset inside the helper's own allocation"""
    n = torch.empty((), dtype=dtype).element_size()
    return t.buf[byte_offset_from_buf_start:byte_offset_from_buf_start + n].view(dtype)


@pytest.mark.parametrize("role", ["out", "in", "ws"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stray_writes_are_seen(role, dtype):
    def make():
        if role == "ws":
            return guarded(40, torch.uint8, CPU, "ws")
        init = torch.ones(5, 8, dtype=dtype) if role == "in" else None
        return guarded((5, 8), dtype, CPU, role, init=init)

    n = torch.empty((), dtype=dtype).element_size()
    # one element before the payload, one after it, and the far end of each guard
    cases = {
        "one element before": lambda t: t.start - n,
        "one element after": lambda t: t.end,
        "far end of the front guard": lambda t: t.start - t.guard,
        "far end of the tail guard": lambda t: t.end + t.guard - n,
    }
    for what, where in cases.items():
        t = make()
        t.verify()
        _elem_view(t, where(t), dtype).fill_(3.0)
        with pytest.raises(AssertionError) as e:
            t.verify()
        assert "guard changed" in str(e.value), what
    # the message gives offsets relative to the payload edge
    t = make()
    _elem_view(t, t.start - n, dtype).fill_(3.0)
    _elem_view(t, t.end, dtype).fill_(3.0)
    p = t.problems()
    assert len(p) == 2
    assert f"offsets {-n} .. -1 relative to the payload start" in p[0]
    assert f"offsets 0 .. {n - 1} relative to the payload end" in p[1]


def test_offsets_name_the_first_and_last_byte():
    t = guarded((3, 4), torch.float32, CPU, "out")
    t.buf[t.end + 8] = 0
    t.buf[t.end + 100] = 0
    t.buf[t.start - 16] = 0
    p = t.problems()
    assert "2 bytes of the tail guard changed, offsets 8 .. 100 relative to the payload end" in p[1]
    assert "1 bytes of the front guard changed, offsets -16 .. -16 relative to the payload start" in p[0]


def test_a_modified_input_payload_is_seen_bitwise():
    x = torch.randn(3, 5)
    x[1, 2] = float("nan")                       # byte comparison: a NaN input is still "unchanged"
    t = guarded(x.shape, x.dtype, CPU, "in", init=x)
    t.verify()
    t.payload[2, 4] += 1.0
    with pytest.raises(AssertionError, match="input payload changed"):
        t.verify()
    t2 = guarded(x.shape, x.dtype, CPU, "in", init=x)
    t2.payload[0, 0] = -t2.payload[0, 0]         # one sign bit
    with pytest.raises(AssertionError, match="input payload changed"):
        t2.verify()
    # an in/out buffer may change; its guards may not
    u = guarded(x.shape, x.dtype, CPU, "inout", init=x)
    u.payload.mul_(2.0)
    u.verify()
    u.buf[u.end] = 0
    with pytest.raises(AssertionError, match="tail guard"):
        u.verify()


def test_collection_verifies_every_member_once():
    g = Guards(CPU)
    a = g.inp(torch.ones(2, 3), name="x")
    b = g.out((2, 3), torch.float32, name="y")
    w = g.ws(64, name="scratch")
    b.payload.copy_(a.payload * 2)
    g.verify_all()
    assert [t.name for t in g.outputs()] == ["y"]
    w.buf[w.end] = 0
    a.payload[0, 0] = 5.0
    with pytest.raises(AssertionError) as e:
        g.verify_all()
    msg = str(e.value)
    assert "scratch" in msg and "x (in" in msg and "y (" not in msg
    with pytest.raises(AssertionError):
        with Guards(CPU) as h:
            o = h.out((4,), torch.float32)
            o.buf[o.start - 1] = 0
    with Guards(CPU) as h:
        h.out((4,), torch.float32).payload.zero_()
    assert guards.FILL_NAN == 0xFF and guards.FILL_OUT_GUARD == 0xA5
