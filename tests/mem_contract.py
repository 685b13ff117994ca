"""Guarded buffers for the tests of the buffer contract (tests/test_gpu_mem_contract.py, tests/test_mem_contract_host.py): every pointer
a test hands to the library lies inside one live allocation, with sentinel regions in front of it and behind it, so that a store one tile,
one row or one element outside the transformed extent lands in memory the test compares afterwards -- bit for bit, through an integer
view (a sentinel that merely compares equal as a float, or a NaN that never does, proves nothing).

A plain module: no conftest, no pytest settings, works on CPU and device tensors alike."""
import math

GUARD_MIN = 64          # elements; a condition, not a measurement: at least this, and at least two rows of the innermost pitch
SENTINEL = -6.02e23     # finite, in range for float32, nothing a transform of the tests' inputs produces


def guard_elems(pitch=1):
    """Elements of each guard region: >= GUARD_MIN and >= two rows of `pitch` elements, rounded up to a multiple of 4 (so that the
    region is a multiple of 16 bytes for every element type and the aligned view starts on a 16-byte boundary)."""
    return (max(GUARD_MIN, 2 * int(pitch)) + 3) // 4 * 4


def _bits(t):
    """A flat integer view of t's bytes (complex: two integers per element)."""
    import torch
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.reshape(-1).view({4: torch.int32, 8: torch.int64}[t.element_size()])


def _parts(t):
    return 2 if t.is_complex() else 1


def _fill(dtype):
    """SENTINEL in every component"""
    return complex(SENTINEL, SENTINEL) if dtype.is_complex else SENTINEL


def guarded(count, dtype, device, offset_elems=0, pitch=1):
    """-> (buf, view): `buf` is one allocation filled with SENTINEL, `view` its `count` elements starting guard_elems(pitch) +
    offset_elems elements in; at least guard_elems(pitch) sentinel elements lie behind the view too.  offset_elems = 0: view.data_ptr()
    is on a 16-byte boundary; offset_elems = 1: exactly one ELEMENT past one (8 bytes for complex64, 16 for complex128 -- which stays
    aligned --, 4 / 8 for float32 / float64).  Element alignment is the contract: there is no smaller offset."""
    import torch
    assert count >= 0 and offset_elems in (0, 1)
    g = guard_elems(pitch)
    buf = torch.full((g + 4 + count + g,), _fill(dtype), dtype=dtype, device=device)
    assert buf.data_ptr() % 16 == 0, "the allocator returned a block that is not 16-byte aligned"
    view = buf[g + offset_elems:g + offset_elems + count]
    if count:
        assert (view.data_ptr() - offset_elems * buf.element_size()) % 16 == 0
    return buf, view


def view_start(buf, view):
    """Index in `buf` of view[0] (from the storage offsets: an empty view has no data pointer worth asking for)."""
    return view.storage_offset() - buf.storage_offset()


def bits_equal(a, b):
    """a and b (same dtype, same number of elements) hold the same bytes."""
    import torch
    return a.dtype == b.dtype and a.numel() == b.numel() and bool(torch.equal(_bits(a.contiguous()), _bits(b.contiguous())))


def guards_intact(buf, view, what=""):
    """Every element of `buf` outside `view` still holds SENTINEL, bit for bit.  On failure the assertion names the first spoiled index
    RELATIVE TO THE VIEW (negative: in front of it; >= view.numel(): behind it) and how many elements are spoiled."""
    import torch
    start, count, parts = view_start(buf, view), view.numel(), _parts(buf)
    assert 0 <= start and start + count <= buf.numel()
    want = _bits(torch.full((1,), _fill(buf.dtype), dtype=buf.dtype))[0].item()
    bits = _bits(buf)
    for lo, hi in ((0, start), (start + count, buf.numel())):
        bad = (bits[lo * parts:hi * parts] != want).nonzero()
        if bad.numel():
            first = lo + int(bad[0].item()) // parts
            raise AssertionError(f"{what}: guard spoiled at index {first - start} relative to the view of {count} elements "
                                 f"({math.ceil(bad.numel() / parts)} elements spoiled on this side; the view starts {start} elements into the buffer)")
    return True
