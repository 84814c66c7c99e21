"""ISA facts of fmx_match.hip, checked on the compiler's output in the style of test_isa_fmx_singlets.py (no GPU needed):
the sweep of muxgl_fmx_match_donors keeps the donor rows of a renormalisation block in flight in registers -- no scratch,
no AGPRs, four waves per SIMD at the default tile -- reads the pileup of a wave-uniform SNP through scalar loads, and
turns a marker outside U(k) into a factor of 1 by a select, not by a branch per factor (written with `&&`, the membership
test guards its load of the read count: 64 scalar branches in the loop body of the default tile)."""
import os
import re

from test_isa import CSRC, isa, kernels

UNR, TILE = 8, 4  # FMM_UNR: SNPs per lane between two renormalisations; the default clusters per wave


def test_constants_match_the_source():
    src = open(os.path.join(CSRC, "fmx_match.hip")).read()
    assert re.search(r"constexpr int FMM_UNR = %d;" % UNR, src)
    assert re.search(r"return t == 1 \|\| t == 2 \|\| t == 4 \|\| t == 8 \? t : %d;" % TILE, src)


def test_sweep_kernels(tmp_path_factory):
    text = isa(tmp_path_factory, "fmx_match")
    ks = kernels(text, "fmm_sweep_kernel")
    assert len(ks) == 29  # VH = 1, 2, 4, 8, 16, 32, 64 x T = 1, 2, 4, 8, and the HWE sweep
    for name, (body, meta) in ks.items():
        assert meta["private_seg_size"] == 0, f"{name}: scratch in the sweep kernel"
        assert meta["num_agpr"] == 0, (name, meta)
        assert "scratch_" not in body and "s_swappc" not in body
    for name, (body, meta) in kernels(text, "ELi%dELb0" % TILE).items():   # the default tile, every donor width
        assert meta["num_vgpr"] <= 128, (name, meta)  # four waves per SIMD
    (name, (body, meta)), = kernels(text, "fmm_sweep_kernelILi64ELi%dELb0" % TILE).items()
    # 64 donors: the three diagonal values of every (SNP, cluster) of a loop step come through scalar loads ...
    assert len(re.findall(r"s_load_dwordx2", body)) >= 3 * UNR * TILE, name
    # ... the donors' triples through vector loads, all of a step side by side ...
    assert len(re.findall(r"global_load_dwordx[24]", body)) >= UNR, name
    # ... and no factor has a branch of its own
    assert len(re.findall(r"s_cbranch", body)) < UNR * TILE, name
    for pat in ("fmm_join_kernel", "fmm_count_kernel"):
        (name, (body, meta)), = kernels(text, pat).items()
        assert meta["private_seg_size"] == 0 and "scratch_" not in body
