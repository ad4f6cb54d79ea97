"""The bindings' side of the operand-window contract (include/cwn_hip.h, "OPERAND WINDOWS"), stated once: pure functions of a
tensor's address, shape and strides (CPU tensors too).  csrc/cwn_check.h (`al4` / `al8` / `al16`) is the entry points' half;
`row_major` / `row_major16` of csrc/cwn_torch_ext.cpp are the compiled binding's twins of `rowmajor` / `rowmajor16`."""
import torch


def ld(t, width=None) -> int:
    """The row stride a descriptor carries: `t.stride(0)`, or -- at most one row -- the width (`t.size(1)` unless given)."""
    return t.stride(0) if t.size(0) > 1 else t.size(1) if width is None else width


def aligned16(t) -> bool:
    """The address test: all there is to a per-column vector or a flat buffer."""
    return t.data_ptr() % 16 == 0


def is_rowmajor(t) -> bool:
    """Unit column stride (> 1 column), rows that do not overlap (> 1 row): a window of a wider matrix, no transposed / column-strided view."""
    return (t.size(1) <= 1 or t.stride(1) == 1) and (t.size(0) <= 1 or t.stride(0) >= t.size(1))


def is_vec16(t, stride=None) -> bool:
    """Rows readable 16 bytes at a time: `aligned16` and a row stride that is a multiple of 4 -- the RECORDED `t.stride(0)`, or
    the `stride` given (`ld(t)`: the two differ for ONE row with an odd recorded stride, `buf[0:1, :64]` of a [1, 67] buffer)."""
    return t.data_ptr() % 16 == 0 and (t.stride(0) if stride is None else stride) % 4 == 0


def rowmajor(t):
    """`t` itself where `is_rowmajor`, else a fresh contiguous copy (an input: an output cannot be copied)."""
    return t if is_rowmajor(t) else t.clone(memory_format=torch.contiguous_format)


def rowmajor16(t, stride=None):
    """`t` itself where `is_rowmajor` and `is_vec16(t, stride)`, else a fresh contiguous copy.  A clone, not `.contiguous()`: ONE
    row of a wider matrix is "contiguous" to torch wherever it starts and whatever its stride says, and would come back as it lies."""
    return t if is_rowmajor(t) and is_vec16(t, stride) else t.clone(memory_format=torch.contiguous_format)
