"""Guarded allocation for the tests: every tensor a factory call makes on one device gets canary bands around it and a poisoned body.

`GuardedAlloc(device, poison)` is a torch.overrides.TorchFunctionMode.  While it is entered, the factory calls the package uses

    torch.empty / zeros / ones / full, their *_like forms, Tensor.new_empty / new_zeros / new_full / new_ones

are answered, when their result would live on `device`, from one uint8 arena each:

    | front band, FRONT bytes of CANARY | body, exactly numel * element_size bytes | back band, BACK bytes of CANARY |

The body holds the poison byte for the `empty` forms and the requested value for the others; the call returns
`arena[FRONT:FRONT + nbytes].view(dtype)` in the shape (and strides) the unguarded call would have given.  Calls for another device,
and every other function, pass through untouched.  The guard keeps every arena alive until it is dropped, so no two guarded tensors
ever share memory and `violations()` can look at all of them at the end.

What the two bytes are for.  The caching allocator rounds every block up to 512 bytes or more, so a kernel that writes a few
elements past its output, or a size query that is a little too small, corrupts nothing a test reads: here the first byte after the
body is a canary.  And torch.empty on a fresh process mostly returns zeros, so a kernel that reads what the call never wrote passes:
here it reads the poison (0xFF: NaN as a float, -1 as an integer, so a stale index lands in the front band and not far away; 0x00:
what fresh memory usually holds, so a difference between the two runs names the dependence).

Band sizes.  FRONT is 4 KiB: a multiple of 512, so a body is aligned as the caching allocator aligns it (and at least as well as any
element size asks).  BACK is 64 KiB and starts at the first byte after the body whatever the body's size.  The plausible overruns of
this project's kernels are a word past a byte row (3 bytes), a pad row of the bit matrix (npad / 8 bytes: 64 KiB covers clouds of up
to 524 288 points, the contract cases use 2086), the last brick or 8^3 tile of a ragged grid (at most 512 cells of 4 bytes) and the
last 2048-point tile of a cloud (2048 rows of 16 bytes = 32 KiB): all inside 64 KiB, so there was no reason to differ.

What it cannot see: allocations made inside an autograd backward node (the engine runs them outside the mode: drive the backward
ops directly), reads out of bounds (they change nothing), overruns inside the internal layout of one workspace (one body),
and writes further than a band away.  A write into the bands is inside memory this module owns: detecting it can never fault.
"""
import os
import sys

import torch
from torch.overrides import TorchFunctionMode

FRONT = 4096
BACK = 65536
CANARY = 0xA5

_EMPTY, _ZEROS, _ONES, _FULL = "empty", "zeros", "ones", "full"
# function -> (kind, index of the fill value among the positional arguments or None, does the first argument give the device?)
_FACTORIES = {
    torch.empty: (_EMPTY, None, False), torch.zeros: (_ZEROS, None, False), torch.ones: (_ONES, None, False),
    torch.full: (_FULL, 1, False),
    torch.empty_like: (_EMPTY, None, True), torch.zeros_like: (_ZEROS, None, True), torch.ones_like: (_ONES, None, True),
    torch.full_like: (_FULL, 1, True),
    torch.Tensor.new_empty: (_EMPTY, None, True), torch.Tensor.new_zeros: (_ZEROS, None, True),
    torch.Tensor.new_ones: (_ONES, None, True), torch.Tensor.new_full: (_FULL, 2, True),
}
_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__)) + os.sep
_THIS_FILE = os.path.abspath(__file__)


def _canonical(device):
    """A device with its index made explicit ('cuda' alone is the current device)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        return torch.device("cuda", torch.cuda.current_device())
    return device


def _call_site():
    """(file, line) of the first frame outside torch and this module."""
    f = sys._getframe(1)
    while f is not None:
        name = os.path.abspath(f.f_code.co_filename)
        if name != _THIS_FILE and not name.startswith(_TORCH_DIR):
            return name, f.f_lineno
        f = f.f_back
    return "?", 0


class Arena:
    __slots__ = ("buf", "nbytes", "site", "kind")

    def __init__(self, buf, nbytes, site, kind):
        self.buf, self.nbytes, self.site, self.kind = buf, nbytes, site, kind


class Violation:
    """One arena whose bands changed: `site` = (file, line) of the factory call, `nbytes` the body's size, `offsets` the changed
    bytes relative to the body's first byte (negative: front band; >= nbytes: back band), ascending."""

    def __init__(self, site, nbytes, offsets, index):
        self.site, self.nbytes, self.offsets, self.index = site, nbytes, offsets, index

    def __repr__(self):
        where = ", ".join(str(o) for o in self.offsets[:8]) + (", ..." if len(self.offsets) > 8 else "")
        return f"{self.site[0]}:{self.site[1]}: body of {self.nbytes} bytes, canary bytes changed at offsets [{where}]"


class GuardedAlloc(TorchFunctionMode):
    def __init__(self, device, poison=0xFF, front=FRONT, back=BACK, canary=CANARY):
        super().__init__()
        assert front % 512 == 0 and front > 0 and back > 0 and 0 <= poison <= 255 and 0 <= canary <= 255
        self.device, self.poison, self.front, self.back, self.canary = _canonical(device), poison, front, back, canary
        self.arenas = []

    # ---- interception -------------------------------------------------------------------------------------------------------
    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        spec = _FACTORIES.get(func)
        if spec is None:
            return func(*args, **kwargs)
        kind, fill_at, like = spec
        device = kwargs.get("device")
        if device is None:
            device = args[0].device if like else torch.get_default_device()
        if _canonical(device) != self.device or kwargs.get("out") is not None or kwargs.get("pin_memory"):
            return func(*args, **kwargs)
        site = _call_site()
        with torch._C.DisableTorchFunction():
            meta = func(*args, **{**kwargs, "device": "meta", "requires_grad": False})   # torch's own reading of the arguments
            if meta.layout != torch.strided:
                return func(*args, **kwargs)
            nbytes = meta.numel() * meta.element_size()
            arena = torch.empty(self.front + nbytes + self.back, dtype=torch.uint8, device=self.device)
            arena[:self.front] = self.canary
            arena[self.front + nbytes:] = self.canary
            body = arena[self.front:self.front + nbytes]
            flat = body.view(meta.dtype)
            if kind == _EMPTY:
                body.fill_(self.poison)
            elif kind == _ZEROS:
                body.zero_()
            elif kind == _ONES:
                flat.fill_(1)
            else:
                flat.fill_(kwargs["fill_value"] if "fill_value" in kwargs else args[fill_at])
            out = flat.as_strided(meta.shape, meta.stride())
        self.arenas.append(Arena(arena, nbytes, site, kind))
        if kwargs.get("requires_grad"):
            out.requires_grad_(True)
        return out

    # ---- the check ----------------------------------------------------------------------------------------------------------
    def violations(self):
        """-> [Violation] of the arenas whose canary bytes changed.  Counted on the device, one small read-back for all arenas; the
        offsets of a damaged arena are read back only when there is one."""
        if not self.arenas:
            return []
        with torch._C.DisableTorchFunction():
            counts = torch.stack([(a.buf[:self.front] != self.canary).sum() + (a.buf[self.front + a.nbytes:] != self.canary).sum()
                                  for a in self.arenas]).cpu()
            out = []
            for i in torch.nonzero(counts).flatten().tolist():
                a = self.arenas[i]
                bad = a.buf != self.canary
                bad[self.front:self.front + a.nbytes] = False
                offsets = (torch.nonzero(bad).flatten() - self.front).cpu().tolist()
                out.append(Violation(a.site, a.nbytes, offsets, i))
        return out

    def owns(self, t):
        """The index of the arena `t` lives in, or None."""
        p = t.untyped_storage().data_ptr()
        for i, a in enumerate(self.arenas):
            if a.buf.untyped_storage().data_ptr() == p:
                return i
        return None
