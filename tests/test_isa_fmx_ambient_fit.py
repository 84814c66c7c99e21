"""ISA facts of fmx_ambient_fit.hip, from the code object's metadata only (no GPU needed, no instruction is inspected), in
the manner of test_isa_fmx_ambient.py: the unit holds one kernel, fam_fit_kernel; it uses no scratch and no AGPRs and stays
within 128 VGPRs (four waves per SIMD) with its nine entry likelihoods and the nine products of a pass (three shares' a_l,
or a, a', a'') in registers."""
from test_isa import isa, kernels


def test_the_fit_kernel_uses_no_scratch_no_agprs_and_at_most_128_vgprs(tmp_path_factory):
    text = isa(tmp_path_factory, "fmx_ambient_fit")
    ks = kernels(text, "fam_fit_kernel")
    assert len(ks) == 1
    assert set(kernels(text, "")) == set(ks)  # every kernel of the unit is this one
    for name, (_body, meta) in ks.items():
        print(name, {k: meta.get(k) for k in ("num_vgpr", "num_agpr", "numbered_sgpr", "private_seg_size")})
        assert meta["private_seg_size"] == 0, f"{name}: scratch"
        assert meta["num_agpr"] == 0, (name, meta)
        assert meta["num_vgpr"] <= 128, (name, meta)
