"""A strict decoder for the FLAC streams this build writes, written from the stream specification in
include/flac/audiocut_flac.h (RFC 9639's layout restricted to what the encoder emits) and independently of the encoder: a
sequential bit reader, no code shared with audio_cut_amd/utils/flac_export.py.  A helper module, not a test; imported by bare name.

`flac_decode(data)` -> (int64 samples [n, channels], info dict).  It raises `FlacError` on anything the specification does not
allow: a wrong marker, a STREAMINFO that does not describe what follows, a bad sync code, a reserved bit set, a frame number out
of sequence, a short frame that is not the last, a wrong CRC-8 or CRC-16, a subframe type other than constant, verbatim or fixed
of order <= 4, wasted bits, a Rice method above 1, an escape parameter, a channel assignment outside the five, padding bits set."""
import numpy as np


class FlacError(ValueError):
    pass


_RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}


def _crc_bitwise(data: bytes, poly: int, width: int, reg: int = 0) -> int:
    top, mask = 1 << (width - 1), (1 << width) - 1
    for byte in data:
        reg ^= byte << (width - 8)
        for _ in range(8):
            reg = ((reg << 1) ^ poly) & mask if reg & top else (reg << 1) & mask
    return reg


_STEP = {(poly, width): [_crc_bitwise(bytes([b]), poly, width) for b in range(256)] for poly, width in ((0x07, 8), (0x8005, 16))}


def _crc(data: bytes, poly: int, width: int) -> int:
    """MSB-first CRC, initial value 0, no reflection; a byte at a time through the 256 single-byte remainders."""
    step, shift, mask, reg = _STEP[(poly, width)], width - 8, (1 << width) - 1, 0
    for byte in data:
        reg = ((reg << 8) & mask) ^ step[(reg >> shift) ^ byte]
    return reg


class _Reader:
    def __init__(self, data: bytes):
        self.text = (np.unpackbits(np.frombuffer(data, dtype=np.uint8)) + 48).astype(np.uint8).tobytes().decode("ascii")   # '0' / '1'
        self.pos = 0

    def take(self, n: int) -> int:
        if self.pos + n > len(self.text):
            raise FlacError("the stream ends inside a field")
        v = int(self.text[self.pos: self.pos + n], 2) if n else 0
        self.pos += n
        return v

    def signed(self, n: int) -> int:
        v = self.take(n)
        return v - (1 << n) if v >> (n - 1) else v

    def words(self, count: int, n: int) -> np.ndarray:
        """`count` signed fields of n bits each, as int64."""
        if self.pos + count * n > len(self.text):
            raise FlacError("the stream ends inside a field")
        bits = np.frombuffer(self.text[self.pos: self.pos + count * n].encode("ascii"), dtype=np.uint8).astype(np.int64) - 48
        self.pos += count * n
        v = bits.reshape(count, n) @ (1 << np.arange(n - 1, -1, -1, dtype=np.int64))
        return np.where(v >> (n - 1) != 0, v - (1 << n), v)

    def rice(self, count: int, k: int) -> list:
        """`count` Rice codes of parameter k: a unary quotient (zeros, then a one) and k low bits each; the folded values."""
        text, pos, out = self.text, self.pos, []
        for _ in range(count):
            at = text.find("1", pos)
            if at < 0:
                raise FlacError("the stream ends inside a unary run")
            u = (at - pos) << k
            pos = at + 1
            if k:
                if pos + k > len(text):
                    raise FlacError("the stream ends inside a field")
                u |= int(text[pos: pos + k], 2)
                pos += k
            out.append(u)
        self.pos = pos
        return out


def _integrate(warm: np.ndarray, res: np.ndarray, order: int) -> np.ndarray:
    """The samples whose order-th finite difference (coefficients 1,-1; 1,-2,1; ...) is `res` from index `order` on and whose
    first `order` samples are `warm`: one running sum per order, each started from the difference the warm-up samples give."""
    d = res
    for j in range(order, 0, -1):
        first = np.diff(warm[:j], n=j - 1)[0]
        d = np.concatenate([[first], first + np.cumsum(d)])
    return d


def _subframe(r: _Reader, block: int, bps: int) -> np.ndarray:
    if r.take(1):
        raise FlacError("subframe padding bit set")
    kind = r.take(6)
    if r.take(1):
        raise FlacError("wasted bits are not part of this stream")
    if kind == 0:
        return np.full(block, r.signed(bps), dtype=np.int64)
    if kind == 1:
        return r.words(block, bps)
    if kind < 8 or kind > 12:
        raise FlacError(f"subframe type {kind:06b}")
    order = kind - 8
    if order >= block:
        raise FlacError(f"fixed order {order} in a block of {block}")
    warm = r.words(order, bps) if order else np.zeros(0, dtype=np.int64)
    method = r.take(2)
    if method > 1:
        raise FlacError(f"residual coding method {method}")
    p = r.take(4)
    if (block >> p) << p != block or (block >> p) <= order:
        raise FlacError(f"partition order {p} in a block of {block}, predictor order {order}")
    folded = []
    for part in range(1 << p):
        k = r.take(4 + method)
        if k == (15 if method == 0 else 31):
            raise FlacError("escape-coded partition")
        folded += r.rice((block >> p) - (order if part == 0 else 0), k)
    u = np.array(folded, dtype=np.int64)
    res = np.where(u & 1, -((u + 1) >> 1), u >> 1)
    out = _integrate(warm, res, order)
    if out.shape[0] != block:
        raise FlacError("a subframe of the wrong length")
    return out


def flac_decode(data: bytes):
    data = bytes(data)
    if data[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    if data[4:8] != bytes([0x80, 0, 0, 34]):
        raise FlacError("the one metadata block must be a last STREAMINFO of 34 bytes")
    if len(data) < 42:
        raise FlacError("STREAMINFO is cut short")
    h = _Reader(data[8:42])
    info = {"min_block": h.take(16), "max_block": h.take(16), "min_frame": h.take(24), "max_frame": h.take(24), "sample_rate": h.take(20),
            "channels": h.take(3) + 1, "bits": h.take(5) + 1, "total": h.take(36), "md5": data[26:42]}
    bs, bits, channels = info["min_block"], info["bits"], info["channels"]
    if info["max_block"] != bs or bs not in (256, 512, 1024, 2048, 4096):
        raise FlacError(f"block sizes {info['min_block']}..{info['max_block']}")
    if bits not in (16, 24) or channels not in (1, 2) or info["sample_rate"] == 0:
        raise FlacError(f"{channels} channel(s) of {bits} bits at {info['sample_rate']} Hz")
    at, number, frames, sizes, got = 42, 0, [], [], 0
    r = body = _Reader(data)
    while at < len(data):
        if got >= info["total"]:
            raise FlacError("bytes behind the last frame")
        r.pos = 8 * at
        if r.take(14) != 0x3FFE:
            raise FlacError(f"no sync code at byte {at}")
        if r.take(1):
            raise FlacError("reserved bit set")
        if r.take(1):
            raise FlacError("variable blocking strategy")
        size_code, rate, assignment, size, reserved = r.take(4), r.take(4), r.take(4), r.take(3), r.take(1)
        if reserved:
            raise FlacError("reserved bit set")
        if size != {16: 4, 24: 6}[bits]:
            raise FlacError(f"sample size code {size:03b} in a {bits}-bit stream")
        if rate != 0 and _RATES.get(rate) != info["sample_rate"] or rate == 0 and info["sample_rate"] in _RATES.values():
            raise FlacError(f"sample-rate code {rate:04b} at {info['sample_rate']} Hz")
        if assignment not in ((0,) if channels == 1 else (1, 8, 9, 10)):
            raise FlacError(f"channel assignment {assignment:04b} with {channels} channel(s)")
        first = r.take(8)
        extra = 0 if first < 0x80 else 1 if first >> 5 == 6 else 2 if first >> 4 == 14 else 3 if first >> 3 == 30 else -1
        if extra < 0:
            raise FlacError("frame number of more than 4 bytes")
        value = first if extra == 0 else first & (0x3F >> extra)
        for _ in range(extra):
            cont = r.take(8)
            if cont >> 6 != 2:
                raise FlacError("bad continuation byte in the frame number")
            value = (value << 6) | (cont & 0x3F)
        if extra != (0 if value < 128 else 1 if value < 2048 else 2 if value < 65536 else 3):
            raise FlacError("frame number not in its shortest form")
        if value != number:
            raise FlacError(f"frame number {value}, expected {number}")
        if 8 <= size_code <= 12:
            block = 256 << (size_code - 8)
        elif size_code == 6:
            block = r.take(8) + 1
            if block - 1 >= 256:
                raise FlacError("8-bit block size field for a long block")
        elif size_code == 7:
            block = r.take(16) + 1
            if block - 1 < 256:
                raise FlacError("16-bit block size field for a short block")
        else:
            raise FlacError(f"block-size code {size_code:04b}")
        if block > bs or (block == bs) != (8 <= size_code <= 12) or (8 <= size_code <= 12 and block != bs):
            raise FlacError(f"a block of {block} samples (code {size_code:04b}) in a stream of block size {bs}")
        if frames and frames[-1].shape[0] != bs:
            raise FlacError("a short frame that is not the last")
        head = r.pos // 8 - at
        if _crc(data[at: at + head], 0x07, 8) != data[at + head]:
            raise FlacError(f"CRC-8 of frame {number}")
        body.pos = 8 * (at + head + 1)
        widths = {0: (bits,), 1: (bits, bits), 8: (bits, bits + 1), 9: (bits + 1, bits), 10: (bits, bits + 1)}[assignment]
        subs = [_subframe(body, block, w) for w in widths]
        pad = -body.pos % 8
        if body.take(pad):
            raise FlacError("padding bits set")
        end = body.pos // 8
        if end + 2 > len(data) or _crc(data[at: end], 0x8005, 16) != int.from_bytes(data[end: end + 2], "big"):
            raise FlacError(f"CRC-16 of frame {number}")
        if assignment == 8:
            subs = [subs[0], subs[0] - subs[1]]
        elif assignment == 9:
            subs = [subs[0] + subs[1], subs[1]]
        elif assignment == 10:
            mid = (subs[0] << 1) | (subs[1] & 1)
            subs = [(mid + subs[1]) >> 1, (mid - subs[1]) >> 1]
        frame = np.stack(subs, axis=1)
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        if frame.min() < lo or frame.max() > hi:
            raise FlacError(f"frame {number} decodes outside {bits} bits")
        frames.append(frame)
        sizes.append(end + 2 - at)
        got += block
        at, number = end + 2, number + 1
    if not frames:
        raise FlacError("no frames")
    if got != info["total"]:
        raise FlacError(f"STREAMINFO promises {info['total']} samples, the frames hold {got}")
    if (min(sizes), max(sizes)) != (info["min_frame"], info["max_frame"]):
        raise FlacError(f"frame sizes {min(sizes)}..{max(sizes)}, STREAMINFO says {info['min_frame']}..{info['max_frame']}")
    info["frames"] = len(frames)
    info["frame_sizes"] = sizes
    return np.concatenate(frames), info
