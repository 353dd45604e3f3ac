"""tests/guard_util.py checked on the CPU (``guarded_empty(..., cpu=True)`` serves CPU requests too): a write outside a
tensor is reported with its guard and offset, the three byte patterns decode as documented, ``same_bits`` sees what
``torch.equal`` does not."""
import math
import struct

import pytest
import torch

from tests import guard_util as gu

DTYPES = (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.complex64)


def test_served_tensors_are_interior_aligned_views_filled_with_the_pattern():
    real = torch.empty
    with gu.guarded_empty(0x7F, cpu=True) as ge:
        assert torch.empty is not real
        a = torch.empty(3, 5, dtype=torch.float32)
        b = torch.empty((7,), dtype=torch.float64, device="cpu")
        c = torch.empty(size=(2, 2), dtype=torch.uint8)
        z = torch.zeros(4)                                   # another factory: passes through
    assert torch.empty is real
    assert ge.served == [((3, 5), torch.float32), ((7,), torch.float64), ((2, 2), torch.uint8)]
    for t in (a, b, c):
        assert t.is_contiguous() and t.data_ptr() % gu.ALIGN == 0
        store = t.untyped_storage()
        front = t.data_ptr() - store.data_ptr()
        assert front >= gu.GUARD_BYTES and store.nbytes() - front - t.numel() * t.element_size() >= gu.GUARD_BYTES
        assert (t.view(torch.uint8) == 0x7F).all()
    assert z.untyped_storage().nbytes() == 16
    assert ge.violations() == []
    with gu.guarded_empty(0xFF) as ge:                       # without the flag CPU requests pass through
        plain = torch.empty(4)
    assert ge.served == [] and plain.untyped_storage().nbytes() == 16


def test_a_write_outside_the_tensor_is_reported_with_its_guard_and_offset():
    with gu.guarded_empty(0xFF, cpu=True) as ge:
        ok = torch.empty(4, 8, dtype=torch.float32)
        ok.zero_()
        past = torch.empty(4, 8, dtype=torch.float32)
        # one row past the end: elements 32 .. 39, bytes 128 .. 159 from the payload's start
        past.as_strided((5, 8), (8, 1))[4].fill_(1.0)
        before = torch.empty(10, dtype=torch.float64)
        # three elements in front: 24 bytes before the payload
        before.as_strided((1,), (1,), before.storage_offset() - 3).fill_(2.0)
    assert ge.violations() == [((4, 8), torch.float32, "back", 128), ((10,), torch.float64, "front", -24)]


def test_guarded_inputs_report_guards_payload_and_take_an_element_offset():
    t = torch.arange(12, dtype=torch.float32).view(3, 4)
    for offset, dtype in ((0, torch.float32), (1, torch.float32), (1, torch.bfloat16), (3, torch.float64), (1, torch.complex64)):
        src = t.to(dtype)
        view, check = gu.guarded(src, 0x7F, offset)
        assert view.is_contiguous() and view.contiguous().data_ptr() == view.data_ptr()
        assert view.data_ptr() % gu.ALIGN == (offset * src.element_size()) % gu.ALIGN
        assert view.data_ptr() % src.element_size() == 0
        assert torch.equal(view, src) and check() == []
    view, check = gu.guarded(t, 0xFF)
    view.as_strided((1,), (1,), view.storage_offset() + 12).fill_(1.0)
    assert check() == [((3, 4), torch.float32, "back", 48)]
    view, check = gu.guarded(t, 0x00)
    view[1, 2] = -1.0
    assert check() == [((3, 4), torch.float32, "payload", 24)]


def _decode(pattern, dtype):
    with gu.guarded_empty(pattern, cpu=True):
        t = torch.empty(4, dtype=dtype)
    return t


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES])
def test_patterns_decode_as_documented(dtype):
    parts = (lambda t: torch.view_as_real(t)) if dtype.is_complex else (lambda t: t)
    assert (parts(_decode(0x00, dtype)) == 0).all()
    assert torch.isnan(parts(_decode(0xFF, dtype))).all()
    seven = parts(_decode(0x7F, dtype)).double()
    if dtype == torch.float16:
        assert torch.isnan(seven).all()                      # 0x7F7F: exponent all ones, a mantissa
    else:
        assert torch.isfinite(seven).all()
        want = {torch.float32: struct.unpack("<f", b"\x7f" * 4)[0], torch.complex64: struct.unpack("<f", b"\x7f" * 4)[0],
                torch.float64: struct.unpack("<d", b"\x7f" * 8)[0],
                torch.bfloat16: struct.unpack("<f", b"\x00\x00\x7f\x7f")[0]}[dtype]
        assert (seven == want).all() and want > 1e38
        if dtype == torch.float32:
            assert math.isclose(want, 3.39e38, rel_tol=2e-3)


def test_same_bits_sees_signed_zeros_and_nan_payloads():
    z, nz = torch.tensor([0.0, 1.0]), torch.tensor([-0.0, 1.0])
    assert torch.equal(z, nz)
    with pytest.raises(AssertionError, match=r"1 of 2 elements differ.*first at \(0,\)"):
        gu.same_bits(z, nz, "zeros")
    nan_a = torch.tensor([0x7FC00000, 0x7FC00001], dtype=torch.int32).view(torch.float32)
    nan_b = torch.tensor([0x7FC00000, 0x7FC00002], dtype=torch.int32).view(torch.float32)
    gu.same_bits(nan_a, nan_a.clone(), "equal NaNs")         # (torch.equal says no)
    assert not torch.equal(nan_a, nan_a.clone())
    with pytest.raises(AssertionError, match=r"first at \(1,\)"):
        gu.same_bits(nan_a, nan_b, "NaN payloads")
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        gu.same_bits(z.to(dtype), z.to(dtype).clone(), "same")
        with pytest.raises(AssertionError, match="differ in their bits"):
            gu.same_bits(z.to(dtype), nz.to(dtype), "zeros")
    c, nc = torch.complex(z, z), torch.complex(z, nz)
    with pytest.raises(AssertionError, match=r"first at \(0, 1\)"):
        gu.same_bits(c, nc, "complex zeros")
    with pytest.raises(AssertionError, match="float32.*float64"):
        gu.same_bits(z, z.double(), "dtypes")
    m = torch.zeros(2, 3)
    n = m.clone()
    n[1, 2] = 1.0
    with pytest.raises(AssertionError, match=r"first at \(1, 2\)"):
        gu.same_bits(m, n, "index")
