"""ISA facts of demux_unknown.hip, checked on the compiler's output in the style of test_isa_singlets.py (no GPU needed):
the sweep kernel of muxgl_demux_unknown keeps two accumulators per alpha of its chunk beside the loads of a block of
entries in flight -- no scratch, no AGPRs, no LDS -- in every instantiation (widths 1 .. 64 of a column block x chunks of
1, 2 and 3 alphas)."""
from test_isa import isa, kernels


def test_sweep_kernel_uses_no_scratch_no_agprs_and_no_lds(tmp_path_factory):
    text = isa(tmp_path_factory, "demux_unknown")
    ks = kernels(text, "unk_sweep_kernel")
    assert len(ks) == 21  # VH = 1, 2, 4, 8, 16, 32, 64 x CH = 1, 2, 3
    for name, (body, meta) in ks.items():
        assert meta["private_seg_size"] == 0, f"{name}: scratch in the sweep kernel"
        assert meta["num_agpr"] == 0, (name, meta)
        assert meta["num_vgpr"] <= 168, (name, meta)  # three waves per SIMD at least
        assert "scratch_" not in body and "s_swappc" not in body
        assert "ds_read" not in body and "ds_write" not in body and meta.get("group_segment_fixed_size", 0) == 0, name
    for pattern in ("unk_emit_kernel", "unk_mean_kernel", "unk_neutral_kernel"):
        ks = kernels(text, pattern)
        assert len(ks) == 1
        for name, (body, meta) in ks.items():
            assert meta["private_seg_size"] == 0 and "scratch_" not in body, name
