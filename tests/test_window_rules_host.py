"""The bindings' side of the operand-window contract, cwn_amd/_window.py, against a truth table written out by hand from the
contract (include/cwn_hip.h, "OPERAND WINDOWS") -- the expectations below are literals, none is computed by the helpers under
test (tests/_windows.py keeps its own `ld` / `aligned16` for the same reason).  The tensors: the five window classes of
tests/_windows.py at 0, 1, 2 and 33 rows and widths 64 and 37, a transposed view and a column-strided view of each shape.  No
GPU: the rules are functions of an address, a shape and strides."""
import pytest
import torch

from cwn_amd import _window as W
from tests._windows import CLASSES

ROWS = (0, 1, 2, 33)
WIDTHS = (64, 37)

# per (width, class): the recorded row stride, "the window starts on 16 bytes" (the buffer does: col0 * 4 bytes decide), and "the
# rows can be read 16 bytes at a time" judged on the RECORDED stride and on the stride a ONE-row descriptor carries (the width)
#                    stride  aligned  vec16(recorded)  vec16(width)
TABLE = {
    (64, 'W0'): (64, True, True, True),
    (64, 'W1'): (72, True, True, True),
    (64, 'W2'): (72, False, False, False),
    (64, 'W3'): (67, True, False, True),        # <- the two forms differ: ONE row of a [1, 67] buffer
    (64, 'W4'): (65, True, False, True),        # <- and here
    (37, 'W0'): (37, True, False, False),
    (37, 'W1'): (45, True, False, False),
    (37, 'W2'): (45, False, False, False),
    (37, 'W3'): (40, True, True, False),        # <- and the other way round: 40 is a multiple of 4, the width 37 is not
    (37, 'W4'): (38, True, False, False),
}


def _window(cls, M, w):
    col0, extra = CLASSES[cls]
    buf = torch.arange(M * (w + extra), dtype=torch.float32).view(M, w + extra)
    assert M == 0 or buf.data_ptr() % 16 == 0
    return buf[:, col0:col0 + w]


def _copied(r, t, what):
    assert r is not t and (t.numel() == 0 or r.data_ptr() != t.data_ptr()), what
    assert r.shape == t.shape and torch.equal(r, t), what
    assert r.is_contiguous() and r.stride() == torch.empty(t.shape).stride(), what       # row-major as torch allocates it
    assert r.numel() == 0 or r.data_ptr() % 16 == 0, what


@pytest.mark.parametrize('w', WIDTHS)
@pytest.mark.parametrize('M', ROWS)
@pytest.mark.parametrize('cls', sorted(CLASSES))
def test_window_classes(cls, M, w):
    stride, aligned, vec_recorded, vec_width = TABLE[w, cls]
    if M == 0:                       # (torch gives a tensor without elements the null address: nothing is read from it)
        aligned, vec_recorded, vec_width = True, stride % 4 == 0, w % 4 == 0
    t = _window(cls, M, w)
    what = f'{cls} [{M}, {w}]'
    want_ld = stride if M > 1 else w
    assert W.ld(t) == want_ld and isinstance(W.ld(t), int), what
    assert W.ld(t, 5) == (stride if M > 1 else 5), what              # (a descriptor with a width of its own)
    assert W.aligned16(t) is aligned, what
    assert W.is_rowmajor(t) is True, what                            # every window of a wider row-major buffer is
    assert W.is_vec16(t) is vec_recorded, what
    vec_ld = vec_recorded if M > 1 else vec_width
    assert W.is_vec16(t, W.ld(t)) is vec_ld, what
    assert W.rowmajor(t) is t, what
    for r, keep in ((W.rowmajor16(t), vec_recorded), (W.rowmajor16(t, want_ld), vec_ld)):
        if keep:
            assert r is t, what
        else:
            _copied(r, t, what)
            # (a fresh copy is 16-byte readable iff its width is a multiple of 4 -- or it has at most one row and is judged by `ld`)
            assert W.is_vec16(r) is (w % 4 == 0), what


@pytest.mark.parametrize('w', WIDTHS)
@pytest.mark.parametrize('M', ROWS)
def test_views_that_are_no_windows(M, w):
    """A transposed view ([w, M] seen as [M, w]: strides (1, M)) is row-major only where it has at most one row -- a column read
    as a row; a column-strided view (every second column: strides (2w, 2)) never is.  Both are copied."""
    tr = torch.arange(w * M, dtype=torch.float32).view(w, M).t()
    cs = torch.arange(M * 2 * w, dtype=torch.float32).view(M, 2 * w)[:, ::2]
    assert tuple(tr.shape) == tuple(cs.shape) == (M, w)
    assert W.is_rowmajor(tr) is (M <= 1), (M, w)
    assert W.is_rowmajor(cs) is False, (M, w)
    assert W.ld(cs) == (2 * w if M > 1 else w) and W.ld(tr) == (1 if M > 1 else w)
    for t, is_rm in ((tr, M <= 1), (cs, False)):
        for r in (W.rowmajor(t), W.rowmajor16(t), W.rowmajor16(t, W.ld(t))):
            if is_rm and r is t:
                continue
            _copied(r, t, (M, w))
            assert W.is_rowmajor(r), (M, w)
    if M <= 1:
        assert W.rowmajor(tr) is tr


def test_one_row_off_16_bytes_is_cloned():
    """ONE row that starts 4 bytes off a 16-byte boundary: torch calls it contiguous and `.contiguous()` hands it back as it lies,
    off 16 bytes; `rowmajor16` clones it, under both forms of the stride rule (`rowmajor` keeps it: it is row-major)."""
    buf = torch.arange(72, dtype=torch.float32).view(1, 72)
    t = buf[:, 1:65]
    assert t.is_contiguous() and t.contiguous() is t and t.data_ptr() % 16 == 4
    assert W.rowmajor(t) is t
    for r in (W.rowmajor16(t), W.rowmajor16(t, W.ld(t))):
        _copied(r, t, 'one row, 4 bytes off')
        assert W.is_vec16(r) and W.is_vec16(r, W.ld(r))


def test_flat_buffers_and_vectors_take_the_address_test():
    v = torch.zeros(16)
    assert W.aligned16(v) is True and W.aligned16(v[4:]) is True
    assert W.aligned16(v[1:]) is False and W.aligned16(v[2:6]) is False
