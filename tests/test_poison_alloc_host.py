"""tests/poison_alloc.py tests itself on CPU tensors: fake wrappers in plain torch, each with ONE planted mistake, must each be
reported with a message that names the allocation; a correct one must pass; the pass-through and restore rules hold."""
import numpy as np
import pytest
import torch

import poison_alloc as PA

N = 37
CPU = torch.device("cpu")


class _FakeHip:
    """What run_three needs of a context, on the CPU.  `to_device` puts the array at the front of a larger zeroed block, so that the
    planted one-element over-read stays inside memory the test owns in the unpoisoned run as well."""
    device = CPU

    def to_device(self, arr, dtype=None):
        t = torch.as_tensor(np.ascontiguousarray(arr))
        big = torch.zeros(t.numel() + 8, dtype=t.dtype)
        big[: t.numel()] = t.reshape(-1)
        return big[: t.numel()].view(t.shape)

    def prefetch_begin(self):
        pass


def _x():
    return np.random.default_rng(0).standard_normal(N).astype(np.float32)


def _elements(t: torch.Tensor, first: int, count: int) -> torch.Tensor:
    """`count` elements of t's STORAGE from element `first` relative to t[0]: how a fake wrapper strays outside its tensor."""
    return torch.as_strided(t, (count,), (1,), storage_offset=t.storage_offset() + first)


def _correct(x):
    out = torch.empty(N, dtype=torch.float32, device=CPU)
    scratch = torch.empty_like(x)
    scratch.copy_(x * 2)
    out.copy_(scratch + 1)
    return out


def _unwritten(x):
    out = torch.empty(N, dtype=torch.float32, device=CPU)
    out[: N - 1] = x[: N - 1] * 2 + 1
    return out


def _scratch_read_first(x):
    out = torch.empty(N, dtype=torch.float32, device=CPU)
    scratch = torch.empty(N, dtype=torch.float64, device=CPU)
    scratch[1:] = 0.0                    # element 0 is read before anyone wrote it
    out.copy_((x.double() + scratch).float())
    return out


def _input_overread(x):
    out = torch.empty((), dtype=torch.float64, device=CPU)
    out.copy_(_elements(x, 0, N + 1).double().sum())
    return out


def test_poison_values_and_alignment():
    with PA.poisoned(0xFF, "cpu") as pa:
        f = torch.empty(5, dtype=torch.float32, device=CPU)
        i = torch.empty((2, 3), dtype=torch.int64, device="cpu")
        z = torch.empty(0, dtype=torch.float64)
        assert bool(torch.isnan(f).all()) and bool((i == -1).all()) and i.shape == (2, 3) and i.is_contiguous() and z.numel() == 0
        assert f.data_ptr() % 512 == pa.registry[0][0].data_ptr() % 512 and len(pa.registry) == 3
        pa.check_guards()
    with PA.poisoned(0x7F, "cpu") as pa:
        f = torch.empty((3, 5), dtype=torch.float32)
        d = torch.empty_like(f, dtype=torch.float64)
        i = torch.empty(4, dtype=torch.int32)
        assert bool(torch.isfinite(f).all()) and float(f[0, 0]) > 3e38 and float(d[0, 0]) > 1e306 and d.shape == (3, 5)
        assert bool((i == 0x7F7F7F7F).all())
        pa.check_guards()


def test_a_correct_wrapper_passes():
    got = PA.run_three(_FakeHip(), lambda up: _correct(up(_x())), "cpu")
    assert torch.equal(got, torch.from_numpy(_x() * 2 + 1))
    PA.run_three(_FakeHip(), lambda up: {"a": (_correct(up(_x())), 3, None), "b": [_x(), "s", 2.5]}, "cpu")


def test_an_unwritten_output_element_is_reported():
    with pytest.raises(AssertionError, match=r"result \(tensor torch.float32 \(37,\)\) differs .* first at byte 14[4-7] of 148"):
        PA.run_three(_FakeHip(), lambda up: _unwritten(up(_x())), "cpu")


def test_a_scratch_buffer_read_before_it_is_written_is_reported():
    with pytest.raises(AssertionError, match=r"result \(tensor torch.float32 \(37,\)\) differs .* first at byte [0-3] of 148"):
        PA.run_three(_FakeHip(), lambda up: _scratch_read_first(up(_x())), "cpu")


def test_an_input_read_one_element_past_its_end_is_reported():
    with pytest.raises(AssertionError, match=r"result \(tensor torch.float64 \(\)\) differs"):
        PA.run_three(_FakeHip(), lambda up: _input_overread(up(_x())), "cpu")


@pytest.mark.parametrize("poison", PA.POISONS)
def test_a_store_past_the_end_is_reported(poison):
    with PA.poisoned(poison, "cpu") as pa:
        torch.empty(3, dtype=torch.int64)
        out = torch.empty((N,), dtype=torch.float32)
        _elements(out, 0, N + 1).copy_(torch.arange(N + 1.0))
        with pytest.raises(AssertionError, match=r"allocation #1 \(torch.float32, shape \(37,\), 148 bytes\).*offset 14[89] relative "
                                                 r"to the view, [01] byte\(s\) past the end"):
            pa.check_guards()


@pytest.mark.parametrize("poison", PA.POISONS)
def test_a_store_before_the_start_is_reported(poison):
    with PA.poisoned(poison, "cpu") as pa:
        out = torch.empty((4, 5), dtype=torch.float64)
        _elements(out.view(-1), -1, 1).fill_(1.0)
        with pytest.raises(AssertionError, match=r"allocation #0 \(torch.float64, shape \(4, 5\), 160 bytes\).*offset -[1-8] relative"):
            pa.check_guards()


def test_the_round_up_tail_is_watched_and_a_far_store_is_the_stated_limit():
    with PA.poisoned(0xFF, "cpu") as pa:
        out = torch.empty(100, dtype=torch.uint8)
        raw = pa.registry[0][0]
        assert raw.numel() == 2 * PA.GUARD + PA.ROUND
        raw[PA.GUARD + 511] = 0
        with pytest.raises(AssertionError, match="offset 511 relative to the view"):
            pa.check_guards()
        assert out.numel() == 100


def test_pass_through_rules():
    real_empty, real_like = torch.empty, torch.empty_like
    with PA.poisoned(0xFF, "cpu") as pa:
        assert torch.empty is not real_empty and torch.empty_like is not real_like
        dst = torch.zeros(6)
        torch.empty(6, out=dst)
        assert bool((dst == 0).all())
        torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)
        torch.empty(3, device="meta")
        torch.empty_like(torch.zeros(4, 6).t())                        # preserve_format of a non-contiguous tensor
        torch.empty_like(torch.zeros(3), device="meta")
        assert pa.registry == []
        if torch.cuda.is_available():
            torch.empty(4, pin_memory=True)
            torch.empty(4, device="cuda")                              # the filter is "cpu" here
            assert pa.registry == []
        torch.empty_like(torch.zeros(4, 6).t(), memory_format=torch.contiguous_format)
        assert len(pa.registry) == 1 and torch.zeros(3).sum() == 0     # torch.zeros is not touched
    assert torch.empty is real_empty and torch.empty_like is real_like
    with PA.poisoned(0x7F, "cuda") as pa:                              # a CPU allocation under the device filter
        torch.empty(5)
        assert pa.registry == []


def test_a_pinned_call_reaches_the_real_allocator_unchanged():
    """pinning needs a device, so the hand-over itself is checked: the arguments arrive at the real function as they were given."""
    pa = PA.PoisonedAllocator(0xFF, "cpu")
    pa.real_empty = lambda *a, **k: ("real", a, k)
    assert pa.empty((4, 2), dtype=torch.int32, pin_memory=True) == ("real", ((4, 2),), {"dtype": torch.int32, "pin_memory": True})
    assert pa.empty(4, out="dst") == ("real", (4,), {"out": "dst"})
    assert pa.registry == []


def test_restored_after_an_exception():
    real_empty, real_like = torch.empty, torch.empty_like
    with pytest.raises(RuntimeError, match="planted"):
        with PA.poisoned(0xFF, "cpu"):
            raise RuntimeError("planted")
    assert torch.empty is real_empty and torch.empty_like is real_like
    with pytest.raises(AssertionError):
        PA.run_three(_FakeHip(), lambda up: _unwritten(up(_x())), "cpu")
    assert torch.empty is real_empty and torch.empty_like is real_like
