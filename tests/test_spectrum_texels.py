"""The spectrum kernel texel by texel.  k_spectrum (ow_spectrum.hip) evaluates the amplitude in a cheaper form than the reference
(ow_device.h spectrum_amplitude_fast: hardware reciprocals, exp2(e log2 x) on v_exp_f32 / v_log_f32, a saturated tanh, the device libm's
atan2f / cosf / expf), and every map, query, buoyancy result and ray hit is computed from the h0 it writes.  A max-norm over the plane is set
by the few texels at the peak while the spectrum spans tens of orders of magnitude, so these tests hold every texel, in the metric of
helpers.spectrum_margins:

    ratio = |a - r| / ((rho + 4 sens) |r| + max(phi max|r|, sqrt(FLT_MIN))) <= 1,   phi = H.SPEC_PHI = 1e-7

phi: a texel below 1e-7 of the plane's maximum moves any output sample by less than 1e-7 of the largest wave -- three orders of magnitude
under the 1e-4 the maps are held to, and below the rounding noise of the FP32 transform that follows -- so below the floor a texel may
differ freely (it must still be finite); sqrt(FLT_MIN) = 1.1e-19: the amplitude is the square root of an FP32 energy that is subnormal
below it (a record whose whole spectrum lies beyond the grid's highest frequency is such dust).  Above the floor the relative budget rho
carries the comparison, widened only where the formulas themselves cannot do better in FP32: by four ulps of theta - angle times
np_twin.direction_ulp_sensitivity, the relative change of |h0| per ulp of that argument, which is unbounded at the wind's null direction
(|cos((theta - angle) / 2)| ~ 1e-5 there; the device's atan2f differs from glibc's by an ulp, and its h0 by 0.3 % at such a texel).
The records are those of helpers.spectrum_records -- the eight presets, the ten range-edge presets and fourteen fuzzed ones (FP64 scalars,
random seeds, non-square tiles) -- in contexts of eight cascades, a different record in every slot, so that every slot's offset into the
h0 / omega planes is read back.  scripts/spectrum_margins.py measures what the bounds (helpers.SPEC_*) are set from;
profiles/spectrum_margins.txt holds one MI355X run."""
import numpy as np
import pytest

import helpers as H
from godotoceanwaves_amd.presets import DEPTH
from oracle import oracle as O

RECORDS = H.spectrum_records()
BATCHES = [RECORDS[b:b + 8] for b in range(0, len(RECORDS), 8)]
SIZES = [128, 256, 512, 1024, 2048]
# k_spectrum vs the oracle: the share of all texel-channels whose error needs the floor term (about four times the worst on the MI355X)
FLOOR_SHARE_ORACLE = 5e-3    # (measured 1.2e-3)


def test_the_records_reach_every_edge():
    """32 records, four contexts of eight; the fuzzed ones include non-square tiles (the only ones that tell tile_x from tile_y) and seeds
    of both signs"""
    assert len(RECORDS) == 32 and all(len(b) == 8 for b in BATCHES)
    fuzzed = [r for name, r in RECORDS if name.startswith("fuzz")]
    assert sum(r["tile_length"][0] != r["tile_length"][1] for r in fuzzed) >= 4
    assert any(r["spectrum_seed"][0] < 0 for r in fuzzed) and any(r["spectrum_seed"][1] < 0 for r in fuzzed)


@pytest.mark.parametrize("n", SIZES)
def test_oracle_omega_is_mirror_symmetric(n):
    """Pass 1 reads omega of the rows y > N/2 from the mirrored texel ((N - x) % N, (N - y) % N) (ow_device.h Pass1::load_raw: "same
    values, shared lines"): correct only if the omega plane is BITWISE symmetric under that mirror.  The oracle's plane is, for every tile
    of the records (non-square ones included) -- the property held where there is no GPU; the device's plane is checked below."""
    for tile in sorted({tuple(r["tile_length"]) for _, r in RECORDS}):
        om = O.omega(n, tile, DEPTH)
        asym = int((om.view(np.uint32) != H.mirror(om).view(np.uint32)).sum())
        assert asym == 0, f"tile {tile}: {asym} omega texels differ from their mirror"


def _check_twin_leg(name, fast, oracle_h0, twin, sens):
    """fast, oracle_h0, twin: [n][n] complex planes of h0(k); sens: np_twin.direction_ulp_sensitivity.  Against the FP64 twin (tests/np_twin.py,
    written from the shader math and not from the oracle), at every texel above the floor:
      (a) the oracle's literal form is within SPEC_RHO_LITERAL of the truth (plus SPEC_ARG_ULPS ulps of theta - angle where the wind's null
          direction makes that ill-conditioned).  An error that the oracle and the kernel SHARE -- a constant, an index, a formula copied
          wrong into both -- agrees with itself in the comparison with the oracle (test_device_spectrum_texel_by_texel) and cannot hide here;
      (b) the kernel's form is at most SPEC_KAPPA times the literal form's own error away from the truth, plus SPEC_RHO_TWIN of |twin| (and the
          same allowance for the null direction): the cheaper form may be worse than the literal one only by that much, texel by texel."""
    if np.abs(twin).max() == 0:
        assert not fast.any() and not oracle_h0.any(), f"{name}: the truth is zero everywhere"
        return
    lo = H.spectrum_margins(oracle_h0[..., None], twin[..., None], H.SPEC_RHO_LITERAL, sens[..., None])
    assert lo["worst"] <= 1.0, f"{name}: oracle vs FP64 twin ratio {lo['worst']:.3g} at (y, x) {lo['at'][:2]} (rho needed {lo['rho_needed']:.2e})"
    extra = H.SPEC_KAPPA * np.abs(oracle_h0 - twin)[..., None]
    m = H.spectrum_margins(fast[..., None], twin[..., None], H.SPEC_RHO_TWIN, sens[..., None], extra=extra)
    assert m["worst"] <= 1.0, f"{name}: kernel vs FP64 twin ratio {m['worst']:.3g} at (y, x) {m['at'][:2]} (rho needed {m['rho_needed']:.2e})"


@pytest.mark.parametrize("n", SIZES)
def test_emulated_kernel_form_against_fp64_truth(n):
    """The twin leg on the CPU: spectrum_amplitude_fast compiled as plain C++ (tests/emul) over glibc's libm, every record, every size.  Guards
    the formulas and the index math where there is no GPU; the device test below guards the instructions."""
    E = H.emul_library()
    pcs = [H.record_pc(r) for _, r in RECORDS]
    for (name, _), pc, (oracle4, twin, _, sens) in zip(RECORDS, pcs, H.spectrum_references(n, pcs)):
        orc, fast, twin = H.zero_where_reference_is_not_finite(H.h0_complex(oracle4)[..., 0], H.emul_fast_h0(E, n, pc), twin)
        _check_twin_leg(name, fast, orc, twin, sens)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", range(len(BATCHES)))
@pytest.mark.parametrize("n", SIZES)
def test_device_spectrum_texel_by_texel(n, batch):
    """k_spectrum's h0 and omega for eight records in the eight slots of one context, read through ow_get_spectrum:
      * the push constants of every slot's launch are the pack of its record (so the references below see the device's inputs);
      * every texel finite where the oracle's is (H.zero_where_reference_is_not_finite: the reference's log(0) of one texel in 2^31);
      * h0 against the oracle's literal form (O.spectrum_compute): ratio <= 1 at rho = SPEC_RHO_ORACLE per texel and channel, the share
        that needs the floor bounded, and the 2e-5 max-norm of test_gpu_parity.test_spectrum_and_omega still held;
      * h0 against the FP64 twin (_check_twin_leg);
      * omega bit-exact against O.omega (at most 2 texels of a plane may differ: double-rounding disagreements, ~2^-28 per texel) and
        BITWISE symmetric under the mirror, which pass 1 relies on (test_oracle_omega_is_mirror_symmetric)."""
    recs = BATCHES[batch]
    pcs = [H.record_pc(r) for _, r in recs]
    dev = H.device_spectra(n, [r for _, r in recs])
    for s, ((name, _), pc, (oracle4, twin, om_ref, sens)) in enumerate(zip(recs, pcs, H.spectrum_references(n, pcs))):
        h0, om, words = dev[s]
        tag = f"{n}^2 slot {s} {name}"
        assert np.array_equal(words[:12], H.pc_words(pc)), f"{tag}: push constants"
        assert np.isfinite(om).all(), tag
        _, twin = H.zero_where_reference_is_not_finite(H.h0_complex(oracle4)[..., 0], twin)
        oracle4, h0 = H.zero_where_reference_is_not_finite(oracle4, h0)
        dev_c, ref_c = H.h0_complex(h0), H.h0_complex(oracle4)
        if np.abs(ref_c).max() == 0:
            assert not h0.any(), f"{tag}: the oracle's spectrum is zero everywhere"
        else:
            m = H.spectrum_margins(dev_c, ref_c, H.SPEC_RHO_ORACLE, np.stack([sens, H.mirror(sens)], axis=-1))
            assert m["worst"] <= 1.0, f"{tag}: ratio {m['worst']:.3g} at (y, x, channel) {m['at']} (rho needed {m['rho_needed']:.2e})"
            assert m["floor_share"] <= FLOOR_SHARE_ORACLE, f"{tag}: {m['floor_share']:.2e} of the texels need the floor"
            assert H.relmax(h0, oracle4) < 2e-5, tag
        _check_twin_leg(tag, dev_c[..., 0], ref_c[..., 0], twin, sens)
        mism = int((om.view(np.uint32) != om_ref.view(np.uint32)).sum())
        assert mism <= 2, f"{tag}: {mism} omega texels differ"
        asym = int((om.view(np.uint32) != H.mirror(om).view(np.uint32)).sum())
        assert asym == 0, f"{tag}: {asym} omega texels differ from their mirror"
