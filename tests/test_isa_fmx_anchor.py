"""ISA facts of fmx_anchor.hip, from the code object's metadata only (no GPU needed), in the manner of
test_isa_fmx_unknown.py: the second writer of the posterior tensor is one small kernel that keeps its row in registers --
no scratch, no LDS."""
from test_isa import isa, kernels


def test_anchor_kernel_uses_no_scratch_and_no_lds(tmp_path_factory):
    text = isa(tmp_path_factory, "fmx_anchor")
    ks = kernels(text, "fmx_anchor_kernel")
    assert len(ks) == 1
    for name, (_body, meta) in ks.items():
        assert meta["private_seg_size"] == 0, f"{name}: scratch"
        assert meta.get("group_segment_fixed_size", 0) == 0, (name, meta)
        assert meta["num_agpr"] == 0 and meta["num_vgpr"] <= 64, (name, meta)
