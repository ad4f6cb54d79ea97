"""Operands laid out as WINDOWS of wider buffers, and the checks that go with them (include/cwn_hip.h, "OPERAND WINDOWS").

An operand [M, w] lives at the columns [col0, col0 + w) of a buffer [M, ld]; a per-column vector [w] at the elements
[off, off + w) of a longer one.  Inputs hold NaN outside the window (a load that strays and is not discarded shows in the
result), outputs hold a sentinel outside it (a store that strays shows).  `Windows` records every buffer it hands out with a
bit image of it, and after the launch
    neighbours()   (c) every element of every output buffer outside its window, and every element of every input buffer,
                       still has its bits;
    no_leak()      (d) no NaN inside a result window.
The same code runs on the CPU over torch emulations of an operation (tests/test_windows_host.py: the checks can fail) and on
the GPU over the kernels (tests/test_gpu_windows.py)."""
import torch

NAN = float('nan')
SENT = -9.0

# window classes: name -> (col0, ld - w)
CLASSES = {
    'W0': (0, 0),      # contiguous
    'W1': (4, 8),      # pointer 16-byte aligned, stride a multiple of 4: the vector form stays eligible
    'W2': (1, 8),      # pointer 4-byte aligned only
    'W3': (0, 3),      # stride not a multiple of 4: every second row is off 16 bytes
    'W4': (0, 1),      # for widths that are no multiple of 4: one element between the rows -- a vector tail that runs over shows
}
VEC_OFF = {'W0': 0, 'W1': 4, 'W2': 1, 'W3': 3, 'W4': 1}      # where a per-column vector starts in its longer buffer
ROWS = (1, 33, 70)     # one row (stride substituted by the width); one past a 32-row tile; two ragged tiles of 64 / 48


def bits(t: torch.Tensor) -> torch.Tensor:
    """The bit image of a float32 / float64 tensor (NaN compares equal to itself, -0 differs from +0)."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


class Windows:
    def __init__(self, device):
        self.device = device
        self.items = []          # (name, buffer, bit image before the launch, mask of the elements the launch may write)

    def _keep(self, name, buf, mask):
        self.items.append((name, buf, bits(buf).clone(), mask))

    def inp(self, name: str, data: torch.Tensor, cls, dtype=torch.float32) -> torch.Tensor:
        """`data` [M, w] as a window of class `cls` (a name of CLASSES or a (col0, ld - w) pair), NaN around it."""
        col0, extra = CLASSES[cls] if isinstance(cls, str) else cls
        M, w = data.shape
        buf = torch.full((M, w + extra), NAN, dtype=dtype)
        buf[:, col0:col0 + w] = data
        buf = buf.to(self.device)
        self._keep(name, buf, None)
        return buf[:, col0:col0 + w]

    def out(self, name: str, M: int, w: int, cls, prefill: torch.Tensor = None, dtype=torch.float32) -> torch.Tensor:
        """An output window: the sentinel everywhere, or `prefill` [M, w] inside the window (accumulated outputs)."""
        col0, extra = CLASSES[cls] if isinstance(cls, str) else cls
        buf = torch.full((M, w + extra), SENT, dtype=dtype)
        if prefill is not None:
            buf[:, col0:col0 + w] = prefill
        buf = buf.to(self.device)
        mask = torch.zeros(M, w + extra, dtype=torch.bool, device=self.device)
        mask[:, col0:col0 + w] = True
        self._keep(name, buf, mask)
        return buf[:, col0:col0 + w]

    def halves(self, name: str, M: int, w: int, cls, parts: int = 2, reverse: bool = False):
        """`parts` output windows of width w side by side in ONE buffer [M, col0 + parts * w + ...] (the halves of a wider
        matrix); `reverse` hands them out in the opposite column order."""
        col0, extra = CLASSES[cls] if isinstance(cls, str) else cls
        buf = torch.full((M, parts * w + extra), SENT).to(self.device)
        mask = torch.zeros(M, parts * w + extra, dtype=torch.bool, device=self.device)
        mask[:, col0:col0 + parts * w] = True
        self._keep(name, buf, mask)
        views = [buf[:, col0 + k * w: col0 + (k + 1) * w] for k in range(parts)]
        return views[::-1] if reverse else views

    def vec(self, name: str, data: torch.Tensor, off: int, out: bool = False) -> torch.Tensor:
        """A per-column vector [w] at the elements [off, off + w) of a NaN-padded (input) / sentinel-padded (output, which holds
        `data` inside the window) longer one."""
        w = data.numel()
        buf = torch.full((off + w + 5,), SENT if out else NAN, dtype=data.dtype)
        buf[off:off + w] = data
        buf = buf.to(self.device)
        mask = None
        if out:
            mask = torch.zeros(off + w + 5, dtype=torch.bool, device=self.device)
            mask[off:off + w] = True
        self._keep(name, buf, mask)
        return buf[off:off + w]

    def neighbours(self, what: str) -> None:
        """(c) outputs: every element outside the window has the bits it had; inputs: every element has."""
        for name, buf, before, mask in self.items:
            changed = bits(buf) != before
            if mask is not None:
                changed = changed & ~mask
            n = int(changed.sum())
            if n:
                where = changed.nonzero()[0].tolist()
                kind = 'an element beside the output window was written' if mask is not None else 'an input buffer was written'
                raise AssertionError(f'{what}: {name}: {kind} ({n} elements, the first at {where})')

    def unchanged(self, what: str) -> None:
        """(e) a refused call: EVERY element of every buffer, the output windows included, has the bits it had."""
        for name, buf, before, _ in self.items:
            n = int((bits(buf) != before).sum())
            assert n == 0, f'{what}: {name}: {n} elements were written by a call that was to write nothing'

    @staticmethod
    def no_leak(view: torch.Tensor, what: str) -> None:
        """(d) no NaN inside a result window."""
        n = int(torch.isnan(view).sum())
        assert n == 0, f'{what}: {n} NaN inside the result window: a neighbour of an input window reached the result'


def aligned16(t: torch.Tensor) -> bool:
    return t.data_ptr() % 16 == 0


def ld(t: torch.Tensor) -> int:
    """The row stride a descriptor carries for a 2-D window (one row: the width)."""
    return t.stride(0) if t.size(0) > 1 else t.size(1)
