"""True-stereo extension: the entry points of include/audiocut_hip_stereo.h refuse bad arguments, and the host side of stereo I/O
(loader, WAV header, frame interleaving, `audio.channels` validation).  CPU only."""
import wave

import numpy as np
import pytest

from abi_surface import lib  # noqa: F401  (the fixture)
from audio_cut_amd.utils import audio_export as AE

SR = 44100


def test_stereo_entry_points_reject_bad_arguments(lib):
    # null context / sizes out of range come back as AC_E_INVALID, never as a launch
    assert lib.ac_mdx_stft_stereo(None, None, 0, None, None, None, 0, None, None, None) == -1
    assert lib.ac_mdx_assemble_ola_stereo(None, None, 0, None, None, None, None, None, None, 0, None, None, None, None, None) == -1
    assert lib.ac_mdx_chunk_vocal_stereo(None, None, 0, None, None, None, None, None, 0, 0, None, None) == -1


def _write_wav(path, frames: np.ndarray, width: int, sr: int = 48000) -> None:
    """frames: float [n, channels] in [-1, 1) -> PCM16 / PCM24 WAV (the values are exact multiples of the step)."""
    if width == 2:
        raw = np.rint(frames * 32768.0).astype("<i2").tobytes()
    else:
        v = np.rint(frames * 8388608.0).astype(np.int32).reshape(-1)
        b = np.empty((v.size, 3), np.uint8)
        b[:, 0] = v & 0xFF; b[:, 1] = (v >> 8) & 0xFF; b[:, 2] = (v >> 16) & 0xFF
        raw = b.tobytes()
    with wave.open(str(path), "wb") as w:
        w.setnchannels(frames.shape[1]); w.setsampwidth(width); w.setframerate(sr); w.writeframes(raw)


@pytest.mark.parametrize("width", [2, 3])
def test_stereo_loader_wav_and_npy(tmp_path, width):
    from audio_cut_amd.api import load_audio_mono, load_audio_stereo
    rng = np.random.default_rng(width)
    step = 2.0 ** (1 - 8 * width)
    frames = np.rint(rng.uniform(-0.9, 0.9, size=(1000, 2)) / step) * step
    _write_wav(tmp_path / "st.wav", frames, width)
    st, sr = load_audio_stereo(str(tmp_path / "st.wav"))
    assert sr == 48000 and st.dtype == np.float32 and st.shape == (2, 1000) and st.flags["C_CONTIGUOUS"]
    assert np.array_equal(st, frames.T.astype(np.float32))
    mono, _ = load_audio_mono(str(tmp_path / "st.wav"))
    assert np.array_equal(mono, np.mean(st, axis=0))                       # the mono loader's mean is the stereo rows' mean
    assert np.array_equal((st[0] + st[1]) * np.float32(0.5), mono)        # = (L + R) * 0.5 in float32, the device's mono mix
    _write_wav(tmp_path / "mono.wav", frames[:, :1], width)
    st1, _ = load_audio_stereo(str(tmp_path / "mono.wav"))                # a mono file goes to both channels
    assert st1.shape == (2, 1000) and np.array_equal(st1[0], st1[1]) and np.array_equal(st1[0], frames[:, 0].astype(np.float32))
    _write_wav(tmp_path / "three.wav", np.repeat(frames[:, :1], 3, axis=1), width)
    with pytest.raises(ValueError):
        load_audio_stereo(str(tmp_path / "three.wav"))
    # .npy: (channels, N) as the mono loader reads it, 1-D duplicated
    x = rng.standard_normal((2, 500)).astype(np.float32)
    np.save(tmp_path / "st.npy", x)
    np.save(tmp_path / "m.npy", x[0])
    got, sr2 = load_audio_stereo(str(tmp_path / "st.npy"))
    assert sr2 == SR and np.array_equal(got, x)
    got1, _ = load_audio_stereo(str(tmp_path / "m.npy"))
    assert np.array_equal(got1, np.stack([x[0], x[0]]))


def test_stereo_wav_header_and_packed_track_interleave(tmp_path):
    rng = np.random.default_rng(5)
    st = rng.uniform(-1.1, 1.1, size=(2, 777)).astype(np.float32)
    pk = AE.PackedTrack(st, SR)                                           # host path (no context)
    assert pk.channels == 2 and pk.n == 777 and pk.width == 3
    inter, _ = AE.pcm_bytes_host(np.stack([st[0], st[1]], axis=1).reshape(-1), "PCM_24")   # L0 R0 L1 R1 ...
    p = pk.write(tmp_path / "seg.wav", 100, 400)
    with wave.open(str(p), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (2, 3, SR, 300)
        assert w.readframes(300) == inter[100 * 6: 400 * 6].tobytes()
    raw = p.read_bytes()
    assert raw[:44] == AE.wav_header(300, SR, 2, 3)
    assert int.from_bytes(raw[22:24], "little") == 2 and int.from_bytes(raw[32:34], "little") == 6   # channels, block align
    assert int.from_bytes(raw[40:44], "little") == 300 * 6
    q = AE.export_audio(st, SR, tmp_path / "full_1.0", "wav")
    assert q.read_bytes() == AE.wav_header(777, SR, 2, 3) + inter.tobytes()
    with pytest.raises(ValueError):
        AE.export_audio(np.zeros((3, 10), np.float32), SR, tmp_path / "x", "wav")
    # mono output is what it was: one channel, the plain packing
    m = AE.export_audio(st[0], SR, tmp_path / "mono", "wav")
    assert m.read_bytes() == AE.wav_header(777, SR, 1, 3) + AE.pcm_bytes_host(st[0], "PCM_24")[0].tobytes()


@pytest.mark.parametrize("value", [0, 3, "2"])
def test_audio_channels_other_than_1_or_2_is_refused(tmp_path, value):
    from audio_cut_amd import api
    from audio_cut_amd import config as cfg
    src = tmp_path / "in.wav"
    _write_wav(src, np.zeros((100, 2)), 2)
    before = cfg.snapshot()
    with pytest.raises(ValueError, match="audio.channels"):
        api.separate_and_segment(input_uri=str(src), export_dir=str(tmp_path / "out"), runtime_overrides={"audio.channels": value})
    assert cfg.snapshot() == before                                        # the runtime overrides were rolled back
