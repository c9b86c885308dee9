"""The exact-by-construction inputs of tests/unet_exact.py, checked on the CPU: every case the GPU file uses passes the helper's own
conditions, the numpy emulation of the split-f16 GEMM reproduces the float64 reference bit for bit on each, and the inputs are not
too tame - each deliberate defect of the emulation changes the result of at least one case of every kernel family."""
import pytest
import torch

import unet_exact as UE

IDS = [c[0] for c in UE.CASES]
AMAX_IDS = [c[0] for c in UE.CASES if c[3] and c[1] in UE.SPLIT_KINDS]


def _grids(case_id):
    return UE.grids_of(UE.CASES[IDS.index(case_id)][1])


@pytest.mark.parametrize("case_id", IDS)
def test_case_is_exact_and_the_emulation_reproduces_float64(case_id):
    """make_case asserts the split / partial-sum / representability conditions itself; the emulation (float16 hi / lo, float32
    accumulation in k-steps of 32, three terms) then equals the float64 reference exactly."""
    for grid in _grids(case_id):
        case = UE.case_of(case_id, grid)
        assert torch.equal(UE.emulate(case), case.ref64), (case_id, grid)


@pytest.mark.parametrize("case_id", AMAX_IDS)
def test_case_with_row_levels_is_exact_at_the_kernels_scale(case_id):
    """rows at different power-of-two levels and the true per-row maximum as in_amax: still exact at the scale the kernel picks."""
    for grid in _grids(case_id):
        case = UE.case_of(case_id, grid, levels=True)
        assert case.in_amax is not None and len(set(case.in_amax[0].tolist())) > 1
        assert torch.equal(UE.emulate(case), case.ref64), (case_id, grid)


def test_x_lo_grid_needs_the_low_part_and_w_lo_grid_the_other():
    case = UE.case_of("conv-one_tile-relu", "xlo")
    _, lo = UE.split16(case.t["x"].numpy())
    assert (lo != 0).mean() > 0.2                       # about a third of the activations carry a low part
    _, lo = UE.split16(case.t["w"].numpy() * UE.CP.weight_scale(case.t["w"].numpy()))
    assert not lo.any()
    case = UE.case_of("conv-one_tile-relu", "wlo")
    _, lo = UE.split16(case.t["w"].numpy() * UE.CP.weight_scale(case.t["w"].numpy()))
    assert (lo != 0).mean() > 0.2
    assert not UE.split16(case.t["x"].numpy())[1].any()


@pytest.mark.parametrize("brk", UE.BREAKS)
def test_each_defect_is_seen_in_every_kernel_family(brk):
    """The emulation with one term dropped, one tap zeroed (convs / down: a tap of the window; GEMMs: one k column), the middle
    k-step of 32 skipped or two output columns swapped differs from the reference on at least one exact case of every family (the
    two dropped-term defects: every split-f16 family; the true-float32 kernels have no such term)."""
    seen = {}
    for case_id, kind, _, _ in UE.CASES:
        fam = UE.FAMILY[kind]
        if kind in UE.F32_KINDS and brk.startswith("drop_"):
            continue
        seen.setdefault(fam, False)
        if seen[fam]:
            continue
        for grid in UE.grids_of(kind):
            case = UE.case_of(case_id, grid)
            if not torch.equal(UE.emulate(case, brk), case.ref64):
                seen[fam] = True
    expect = set(UE.FAMILY[k] for k in (UE.SPLIT_KINDS if brk.startswith("drop_") else UE.SPLIT_KINDS + UE.F32_KINDS))
    assert set(seen) == expect and all(seen.values()), seen


@pytest.mark.parametrize("brk,grid", [("drop_xl_wh", "xlo"), ("drop_xh_wl", "wlo")])
def test_each_cross_term_is_pinned_by_its_own_grid(brk, grid):
    """x-lo inputs see a lost xl*wh and are blind to a lost xh*wl (the weights have no low part), w-lo inputs the reverse: the two
    grids pin the two cross terms separately, in every split-f16 family."""
    other = "wlo" if grid == "xlo" else "xlo"
    for fam in sorted(set(UE.FAMILY[k] for k in UE.SPLIT_KINDS)):
        ids = [c[0] for c in UE.CASES if UE.FAMILY[c[1]] == fam]
        assert any(not torch.equal(UE.emulate(UE.case_of(i, grid), brk), UE.case_of(i, grid).ref64) for i in ids[:4]), fam
        assert all(torch.equal(UE.emulate(UE.case_of(i, other), brk), UE.case_of(i, other).ref64) for i in ids[:2]), fam


def test_dropped_terms_on_gaussian_inputs_at_the_old_tolerance():
    """What tests/test_unet_gpu.py's 2e-6 peak-relative tolerance makes of the two dropped-term defects on Gaussian inputs, at the
    smallest shape of each split-f16 kernel.  Measured with the emulation: a lost cross term is 1.7e-4 .. 2.8e-4 of the peak (the
    term is ~2^-12 of each product, the sums grow like sqrt(K)), the intact emulation 1.4e-7 .. 2.4e-7 - so the old tolerance DOES see
    a cross term that is lost everywhere, by two orders of magnitude.  What a tolerance cannot do is tell a defect BELOW 2e-6 of the
    peak (one wrong low-part element in a long sum, a contribution that is small at the shapes tested) from rounding - on the exact
    grids any such defect is a nonzero difference."""
    errs = {}
    for case_id in ("conv-one_tile-relu", "conv_s8-one_tile-relu", "conv_w96-one_tile-relu", "first-c0_4-ci48-one_tile",
                    "tdf-min-N96", "down-ci8-co96-B3", "up-ci20-co72-B3"):
        case = UE.case_of(case_id, "gauss")
        peak = float(case.ref64.abs().max())
        e = {b: float((UE.emulate(case, b) - case.ref64).abs().max()) / peak for b in (None, "drop_xl_wh", "drop_xh_wl")}
        errs[case_id] = e
        print(case_id, {str(k): f"{v:.1e}" for k, v in e.items()})
        assert e[None] < 2e-6, (case_id, e)
        assert e["drop_xl_wh"] > 2e-6 and e["drop_xh_wl"] > 2e-6, (case_id, e)
