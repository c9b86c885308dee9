"""The signals and sample counts the FLAC tests share (a helper module, not a test; imported by bare name): float32 tracks that
reach every subframe type, both Rice methods, the extreme words and all four stereo assignments."""
import numpy as np

SR = 44100
COUNTS = (1, 2, 5, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5)


def mono_signals(n: int, seed: int = 0):
    """[(name, float32 [n])]"""
    rng = np.random.default_rng(seed + n)
    t = np.arange(n)
    impulse = np.zeros(n)
    impulse[n // 2] = 1.0                                                   # one full-scale sample in silence: long unary runs, k > 14
    return [(name, np.asarray(x, dtype=np.float32)) for name, x in (
        ("silence", np.zeros(n)),                                           # constant subframes
        ("dc", np.full(n, 0.25)),
        ("sine", 0.5 * np.sin(2 * np.pi * 440.0 * t / SR)),
        ("noise", rng.uniform(-0.9, 0.9, n)),                               # verbatim, or 5-bit parameters at 24 bits
        ("saturated", rng.choice([-1.5, 1.5], n)),                          # the extreme words
        ("alternating", np.where(t % 2 == 0, 1.0, -1.0)),                   # the largest order-4 residuals
        ("impulse", impulse))]


def stereo_signals(n: int, seed: int = 0):
    """[(name, float32 [n, 2])]: frames of (L, R)."""
    m = dict(mono_signals(n, seed))
    other = np.random.default_rng(seed + 7 * n + 1).uniform(-0.9, 0.9, n).astype(np.float32)
    return [(name, np.stack([left, right], axis=1)) for name, left, right in (
        ("equal", m["sine"], m["sine"]),                                    # side is constant zero
        ("opposite", m["sine"], -m["sine"]),
        ("independent", m["noise"], other),
        ("near", m["sine"], (m["sine"] + 0.01 * other).astype(np.float32)),  # a small side: left/side or mid/side
        ("extreme", m["saturated"], m["alternating"]),                     # side needs all 25 (17) bits
        ("impulse_silence", m["impulse"], m["silence"]))]


def signals(n: int, channels: int, seed: int = 0):
    return mono_signals(n, seed) if channels == 1 else stereo_signals(n, seed)
