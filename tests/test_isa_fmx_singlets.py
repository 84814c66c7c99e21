"""ISA facts of fmx_singlets.hip, checked on the compiler's output in the style of test_isa_singlets.py (no GPU needed): the
sweep kernel of muxgl_fmx_singlets is bound by its gathers of cluster-posterior rows, so it must keep the loads of a
renormalisation block in flight in registers -- no scratch, no AGPRs, four waves per SIMD -- in every instantiation (one
per width of a cluster block, 1 .. 64)."""
import re

from test_isa import isa, kernels

UNR = 8  # FSG_UNR: entries per lane between two renormalisations


def test_constant_matches_the_source():
    import os

    from test_isa import CSRC

    src = open(os.path.join(CSRC, "fmx_singlets.hip")).read()
    assert re.search(r"constexpr int FSG_UNR = %d;" % UNR, src)


def test_sweep_kernel_uses_no_scratch_and_no_agprs(tmp_path_factory):
    text = isa(tmp_path_factory, "fmx_singlets")
    ks = kernels(text, "fsg_sweep_kernel")
    assert len(ks) == 7  # KH = 1, 2, 4, 8, 16, 32, 64
    for name, (body, meta) in ks.items():
        assert meta["private_seg_size"] == 0, f"{name}: scratch in the sweep kernel"
        assert meta["num_agpr"] == 0, (name, meta)
        assert meta["num_vgpr"] <= 128, (name, meta)  # four waves per SIMD at least
        assert "scratch_" not in body and "s_swappc" not in body
        # the posterior rows of a block's entries, loaded side by side
        assert len(re.findall(r"global_load_dwordx[24]", body)) >= UNR, name
    js = kernels(text, "table_join_kernel")
    assert len(js) == 1
    for name, (body, meta) in js.items():
        assert meta["private_seg_size"] == 0 and "scratch_" not in body
