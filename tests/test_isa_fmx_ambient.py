"""ISA facts of fmx_ambient.hip, from the code object's metadata only (no GPU needed, no instruction is inspected), in the
manner of test_isa_fmx_unknown.py: no kernel of the unit uses scratch, and the sweeps of muxgl_fmx_ambient keep the loads
of a renormalisation block in flight in registers -- no AGPRs, no LDS, at most 128 VGPRs (four waves per SIMD) -- in every
instantiation: seven widths of a cluster block (1 .. 64) times the four sizes of a rho chunk (1 .. 4)."""
from test_isa import isa, kernels


def test_no_kernel_uses_scratch_and_the_sweeps_stay_in_128_vgprs(tmp_path_factory):
    text = isa(tmp_path_factory, "fmx_ambient")
    ks = kernels(text, "ambient_sweep_kernel")
    assert len(ks) == 28  # KH = 1, 2, 4, 8, 16, 32, 64 x CH = 1, 2, 3, 4
    for name, (_body, meta) in ks.items():
        assert meta["private_seg_size"] == 0, f"{name}: scratch in a sweep kernel"
        assert meta["num_agpr"] == 0, (name, meta)
        assert meta["num_vgpr"] <= 128, (name, meta)
        assert meta.get("group_segment_fixed_size", 0) == 0, (name, meta)
    wk = kernels(text, "fam_weight_kernel")
    assert len(wk) == 3  # RC = 4, 8, 16
    ek = kernels(text, "ambient_emit_kernel")
    assert len(ek) == 1
    seen = {**ks, **wk, **ek}
    assert set(kernels(text, "")) == set(seen)  # every kernel of the unit is one of these
    for name, (_body, meta) in seen.items():
        assert meta["private_seg_size"] == 0, f"{name}: scratch"
        print(name, {k: meta.get(k) for k in ("num_vgpr", "num_agpr", "numbered_sgpr", "private_seg_size", "group_segment_fixed_size")})
