"""ISA facts of demux_singlets.hip, checked on the compiler's output in the style of test_isa.py (no GPU needed): the
sweep kernel of muxgl_demux_singlets is bound by its gathers of genotype rows, so it must keep its loads in flight in
registers -- no scratch, no AGPRs -- in every instantiation (one per width of a sample block, 1 .. 64)."""
import re

from test_isa import isa, kernels


def test_sweep_kernel_uses_no_scratch_and_no_agprs(tmp_path_factory):
    text = isa(tmp_path_factory, "demux_singlets")
    ks = kernels(text, "sng_sweep_kernel")
    assert len(ks) == 7  # VH = 1, 2, 4, 8, 16, 32, 64
    for name, (body, meta) in ks.items():
        assert meta["private_seg_size"] == 0, f"{name}: scratch in the sweep kernel"
        assert meta["num_agpr"] == 0, (name, meta)
        assert meta["num_vgpr"] <= 128, (name, meta)  # four waves per SIMD at least
        assert "scratch_" not in body and "s_swappc" not in body
        assert len(re.findall(r"global_load_dwordx[24]", body)) >= 8, name  # the entries of a block, loaded side by side
    js = kernels(text, "table_join_kernel")
    assert len(js) == 1
    for name, (body, meta) in js.items():
        assert meta["private_seg_size"] == 0
