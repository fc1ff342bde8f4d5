"""tests/rows_gpu_harness.py without a device: the guarded output buffer and its check, which hold the row libraries' kernels to their
buffer contract, are held to what they claim.  smfft_amd is stood in for by numpy memory (tests/host_device.py) and a kernel by a Python
function that writes through the payload's address.

At 4-byte and 8-byte elements, count = 7, the payload at its front guard and 3 elements behind it: an honest writer passes and gets its
values back; one element written in front of the payload, one behind it, or one left at the prefill fail, each with the message that
names the fault; finite=False lets a written NaN through."""
import numpy as np
import pytest

from tests import rows_gpu_harness as rh
from tests.fir_gpu_harness import GUARD
from tests.host_device import HOST
from tests.host_device import at as _at

COUNT = 7
CASES = [(dtype, front) for dtype in (np.float32, np.complex64) for front in (0, 3)]


def _written(dtype, front, skip=(), also=(), value=None):
    """a guarded buffer whose kernel has written random values, or `value`, to the payload's elements but `skip`, and to the
    elements `also` (indices relative to the payload's base, outside it); returns (buffer, the values)"""
    e = np.dtype(dtype).itemsize
    values = rh.rand(np.random.default_rng(3 + e + front), COUNT, dtype)
    if value is not None:
        values[:] = value
    buf, ptr = rh.guarded(HOST, COUNT, e, front)
    base = ptr - buf.ptr
    assert buf.nbytes == (GUARD + front + COUNT + GUARD) * e and base == (GUARD + front) * e
    assert np.all(buf.mem[:base] == 0x5A) and np.all(buf.mem[base:base + COUNT * e] == 0xFF) and np.all(buf.mem[base + COUNT * e:] == 0x5A)
    for i in sorted(set(range(COUNT)) - set(skip) | set(also)):
        _at(ptr + i * e, dtype, 1)[0] = values[i % COUNT]
    return buf, values


@pytest.mark.parametrize("dtype,front", CASES)
def test_an_honest_writer_passes(dtype, front):
    buf, values = _written(dtype, front)
    got = rh.collect(buf, COUNT, dtype, front)
    assert got.dtype == dtype and got.shape == (COUNT,) and np.array_equal(rh.bits(got), rh.bits(values))


@pytest.mark.parametrize("dtype,front", CASES)
def test_a_write_in_front_of_the_payload_fails(dtype, front):
    buf, _ = _written(dtype, front, also=[-front - 1])
    with pytest.raises(AssertionError, match="in front of its output"):
        rh.collect(buf, COUNT, dtype, front)


@pytest.mark.parametrize("dtype,front", CASES)
def test_a_write_behind_the_payload_fails(dtype, front):
    buf, _ = _written(dtype, front, also=[COUNT])
    with pytest.raises(AssertionError, match="past its output"):
        rh.collect(buf, COUNT, dtype, front)


@pytest.mark.parametrize("dtype,front", CASES)
def test_an_unwritten_element_fails(dtype, front):
    buf, _ = _written(dtype, front, skip=[COUNT - 1])
    with pytest.raises(AssertionError, match="outputs left unwritten"):
        rh.collect(buf, COUNT, dtype, front)
    assert np.all(np.isnan(rh.collect(buf, COUNT, dtype, front, finite=False)[-1:].view(np.float32)))


@pytest.mark.parametrize("dtype,front", CASES)
def test_finite_false_lets_a_written_nan_through(dtype, front):
    buf, _ = _written(dtype, front, value=np.nan)
    with pytest.raises(AssertionError, match="outputs left unwritten"):
        rh.collect(buf, COUNT, dtype, front)
    got = rh.collect(buf, COUNT, dtype, front, finite=False)
    assert got.shape == (COUNT,) and np.all(np.isnan(got.view(np.float32).reshape(COUNT, -1)[:, 0]))


def test_upload_and_the_worst_figures():
    a = rh.rand(np.random.default_rng(5), (3, 5))[:, ::2]            # 4-byte elements, an odd count, not contiguous
    buf = rh.upload(HOST, a)
    assert buf.nbytes == a.nbytes and np.array_equal(buf.to_host(np.float32, a.shape), a)
    worst = rh.Worst()
    assert worst.record(512, np.array([1e-7, 3e-7]), np.array([2e-6])) == [3e-7, 2e-6]
    assert worst.record(512, np.array([2e-7]), np.array([4e-6, 1e-6])) == [3e-7, 4e-6]
    assert worst.record("power", np.array([1e-8]), np.array([1e-8])) == [1e-8, 1e-8] and sorted(worst.seen, key=str) == [512, "power"]
