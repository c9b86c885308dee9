"""bench.py generates its tracks on a thread pool while the weights load: every generator call must give the same array
on a pool as alone, so the timed steps see the same inputs whichever thread made them.  CPU only (short tracks)."""
from concurrent.futures import ThreadPoolExecutor

from audio_cut_amd.testing import signals


def _same(make, seeds, workers):
    serial = [make(sd) for sd in seeds]
    with ThreadPoolExecutor(max_workers=workers) as pool:
        futures = [pool.submit(make, sd) for sd in seeds]
        pooled = [f.result() for f in futures]
    assert all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(serial, pooled))


def test_c2_tracks_on_a_pool_are_the_serial_tracks():
    _same(lambda sd: signals.c2_song(12.0, seed=sd), [2, 100, 101, 102, 50, 51], 4)


def test_c5_tracks_on_a_pool_are_the_serial_tracks():
    # c5_long_form runs its sections on a pool of its own: the bench nests it inside the track pool
    _same(lambda sd: signals.c5_long_form(7.0, seed=sd, section_s=2.0), [5, 6, 50], 3)

