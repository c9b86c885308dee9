"""Poisoned device allocations with guard bands (a helper module, not a conftest).

`poisoned(byte)` replaces `torch.empty` and `torch.empty_like` for its duration (through pytest's MonkeyPatch, so both are restored
on exit, also after an exception).  Every device allocation of `nbytes` becomes the middle of a uint8 block of
GUARD + round_up(nbytes, 512) + GUARD bytes from the real `torch.empty`, the whole block filled with one poison byte; the block and
`nbytes` go into a registry and the caller gets a contiguous view of the requested dtype and shape.  GUARD is a multiple of 512, so
the view is aligned like a fresh allocation (wrappers that carve several arrays out of one buffer rely on that).

  0xFF: floats are NaN, integers -1.         0x7F: floats are huge but finite (3.4e38 / 1.4e306), integers large and positive.

`check_guards()` synchronises and asserts that both guards and the round-up tail of every registered block still hold the poison
byte.  `run_three(hip, fn)` runs `fn(upload)` unpoisoned, under 0xFF and under 0x7F and asserts the three results bit-identical:
an output byte the kernel never writes differs between the two poisoned runs; an uninitialised read that reaches a result differs
between them or turns it into NaN; with `guarded_upload` the bytes around an input are poison too, so a read outside an input that
reaches a result shows the same way.

Limits: a stray store more than GUARD = 4096 bytes away from its allocation is not seen; a read outside an input that does not
reach a result is not seen; memory PyTorch's own operators allocate, and `torch.zeros` / `torch.full` buffers, are not touched.
Calls that pass through unchanged: `pin_memory=True`, `out=`, a non-contiguous memory format, a non-strided layout, and any target
other than the filtered device type."""
import contextlib
import hashlib

import numpy as np
import pytest
import torch

GUARD = 4096            # bytes of poison on either side of every allocation
ROUND = 512             # the caching allocator's granule: an allocation is rounded up to it, the tail is watched too
POISONS = (0xFF, 0x7F)


class PoisonedAllocator:
    def __init__(self, poison: int, device_type: str = "cuda"):
        self.poison = int(poison)
        self.device_type = device_type
        self.real_empty = torch.empty
        self.real_empty_like = torch.empty_like
        self.registry = []          # (raw uint8 block, nbytes, dtype, shape)

    # -- the allocation ---------------------------------------------------------------------------------
    def alloc(self, shape, dtype, device) -> torch.Tensor:
        shape = tuple(int(s) for s in shape)
        nbytes = self.real_empty((), dtype=dtype, device="meta").element_size() * int(np.prod(shape, dtype=np.int64))
        body = -(-nbytes // ROUND) * ROUND
        raw = self.real_empty(GUARD + body + GUARD, dtype=torch.uint8, device=device)
        raw.fill_(self.poison)
        self.registry.append((raw, nbytes, dtype, shape))
        return raw[GUARD: GUARD + nbytes].view(dtype).view(shape)

    def _wants(self, device) -> bool:
        dev = torch.device(device) if device is not None else torch.get_default_device()
        return dev.type == self.device_type

    def empty(self, *size, **kw):
        if (kw.get("pin_memory") or kw.get("out") is not None or kw.get("names") is not None
                or kw.get("memory_format", torch.contiguous_format) is not torch.contiguous_format
                or kw.get("layout", torch.strided) is not torch.strided or not self._wants(kw.get("device"))):
            return self.real_empty(*size, **kw)
        if "size" in kw:
            size = (kw["size"],)
        shape = size[0] if len(size) == 1 and not isinstance(size[0], int) else size
        dtype = kw.get("dtype") or torch.get_default_dtype()
        out = self.alloc(shape, dtype, kw.get("device") if kw.get("device") is not None else torch.get_default_device())
        return out.requires_grad_() if kw.get("requires_grad") else out

    def empty_like(self, x, **kw):
        fmt = kw.get("memory_format", torch.preserve_format)
        plain = fmt is torch.contiguous_format or (fmt is torch.preserve_format and x.is_contiguous())
        device = kw.get("device") if kw.get("device") is not None else x.device
        if (not plain or kw.get("pin_memory") or kw.get("layout", x.layout) is not torch.strided or x.layout is not torch.strided
                or not self._wants(device)):
            return self.real_empty_like(x, **kw)
        out = self.alloc(x.shape, kw.get("dtype") or x.dtype, device)
        return out.requires_grad_() if kw.get("requires_grad") else out

    # -- the check --------------------------------------------------------------------------------------
    def check_guards(self) -> None:
        """Both guards and the round-up tail of every block registered so far still hold the poison byte (synchronises first)."""
        if self.device_type == "cuda":
            torch.cuda.synchronize()
        if not self.registry:
            return
        p = self.poison
        dirty = torch.stack([(raw[:GUARD] != p).any() | (raw[GUARD + nbytes:] != p).any() for raw, nbytes, _, _ in self.registry])
        for index in torch.nonzero(dirty.cpu()).reshape(-1).tolist():
            raw, nbytes, dtype, shape = self.registry[index]
            host = raw.cpu().numpy()
            host[GUARD: GUARD + nbytes] = p
            first = int(np.flatnonzero(host != p)[0]) - GUARD
            where = f"{-first} byte(s) before the start" if first < 0 else f"{first - nbytes} byte(s) past the end (byte {first} of {nbytes})"
            raise AssertionError(f"guard damaged around allocation #{index} ({dtype}, shape {shape}, {nbytes} bytes) under poison "
                                 f"0x{p:02X}: first damaged byte at offset {first} relative to the view, {where}")


@contextlib.contextmanager
def poisoned(poison: int, device_type: str = "cuda"):
    """`with poisoned(0xFF) as pa:` - every `torch.empty` / `torch.empty_like` on a device of `device_type` is guarded and poisoned;
    `pa.check_guards()` at any time.  Both functions are the originals again after the block, also after an exception."""
    pa = PoisonedAllocator(poison, device_type)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch, "empty", pa.empty)
        mp.setattr(torch, "empty_like", pa.empty_like)
        yield pa


def guarded_upload(hip, array, dtype=None) -> torch.Tensor:
    """A host array (or CPU tensor) copied into a view from the poisoned allocator: inside `poisoned`, the bytes around this INPUT
    are poison too.  `hip` only lends its `.device`."""
    t = array if isinstance(array, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(array))
    if dtype is not None:
        t = t.to(dtype)
    dev = torch.empty(tuple(t.shape), dtype=t.dtype, device=hip.device)
    dev.copy_(t)
    return dev


# -- results as bytes ---------------------------------------------------------------------------------------
def flatten(obj, path="result"):
    """[(path, description, bytes)] of a tensor, numpy array, scalar, str, None, or tuple / list / dict of them."""
    if isinstance(obj, torch.Tensor):
        return [(path, f"tensor {obj.dtype} {tuple(obj.shape)}", obj.detach().cpu().contiguous().numpy().tobytes())]
    if isinstance(obj, np.ndarray):
        if obj.dtype == object:
            return flatten(list(obj), path)
        return [(path, f"array {obj.dtype} {obj.shape}", np.ascontiguousarray(obj).tobytes())]
    if isinstance(obj, dict):
        out = [(path, "dict", repr(sorted(obj, key=repr)).encode())]
        for k in sorted(obj, key=repr):
            out += flatten(obj[k], f"{path}[{k!r}]")
        return out
    if isinstance(obj, (tuple, list)):
        out = [(path, "sequence", str(len(obj)).encode())]
        for i, v in enumerate(obj):
            out += flatten(v, f"{path}[{i}]")
        return out
    if obj is None or isinstance(obj, (str, bytes)):
        return [(path, type(obj).__name__, obj if isinstance(obj, bytes) else repr(obj).encode())]
    if isinstance(obj, (bool, int, float, complex, np.generic)):
        a = np.asarray(obj)
        return [(path, f"scalar {a.dtype}", a.tobytes() if a.dtype != object else repr(obj).encode())]
    raise TypeError(f"{path}: cannot compare a {type(obj).__name__} bit for bit")


def _first_difference(a: bytes, b: bytes) -> int:
    if len(a) != len(b):
        return min(len(a), len(b))
    x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    return int(np.flatnonzero(x != y)[0])


def assert_same(runs, names) -> None:
    base = runs[0]
    for other, name in zip(runs[1:], names[1:]):
        assert [(p, d) for p, d, _ in base] == [(p, d) for p, d, _ in other], \
            f"the {name} run returned another structure than the {names[0]} run: {[(p, d) for p, d, _ in other]}"
        for (path, desc, x), (_, _, y) in zip(base, other):
            if x != y:
                at = _first_difference(x, y)
                n_diff = int((np.frombuffer(x, np.uint8) != np.frombuffer(y, np.uint8)).sum()) if len(x) == len(y) else -1
                raise AssertionError(f"{path} ({desc}) differs between the {names[0]} and the {name} run: first at byte {at} of "
                                     f"{len(x)}, {n_diff} byte(s) differ (sha1 {hashlib.sha1(x).hexdigest()[:10]} vs "
                                     f"{hashlib.sha1(y).hexdigest()[:10]}) - an unwritten output, or a read of memory nobody wrote")


def run_three(hip, fn, device_type: str = "cuda"):
    """`fn(upload)` unpoisoned (upload = hip.to_device, the real allocator), under 0xFF and under 0x7F (upload = guarded_upload);
    `hip.prefetch_begin()` before each so that no run is served from the prefetch cache; guards checked after each poisoned run;
    the three results bit-identical.  Returns the unpoisoned result."""
    hip.prefetch_begin()
    clean = fn(hip.to_device)
    runs, names = [flatten(clean)], ["unpoisoned"]
    for p in POISONS:
        with poisoned(p, device_type) as pa:
            hip.prefetch_begin()
            got = fn(lambda a, dtype=None: guarded_upload(hip, a, dtype))
            pa.check_guards()
            runs.append(flatten(got))
            names.append(f"0x{p:02X}-poisoned")
            hip.prefetch_begin()                # drop entries that hold guarded memory
        del got, pa
    assert_same(runs, names)
    return clean
