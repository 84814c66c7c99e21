"""ISA facts of fmx_pairs.hip, checked on the compiler's output in the style of test_isa_fmx_match.py (no GPU needed): the
sweep of muxgl_fmx_cluster_pairs keeps the partner rows of a renormalisation block in flight in registers -- no scratch, no
AGPRs, no more VGPRs than DESIGN.md 4.2f records -- reads the row cluster's pileup, both membership words and af of a
wave-uniform SNP through scalar loads, and turns a marker outside U(a) n U(b) into a factor of 1 by a select, not by a
branch per factor (written with `&&`, the membership test would guard its load of the row cluster's word)."""
import os
import re

from test_isa import CSRC, isa, kernels

UNR, TILES = 8, (4, 8)   # FCP_UNR: SNPs per lane between two renormalisations; the row clusters per wave, the default first
WIDTHS = (2, 4, 8, 16, 32, 64)
# the compiler's VGPR counts, (KH < 64, KH = 64) per tile size: the figures of DESIGN.md 4.2f
VGPR = {4: (210, 166), 8: (246, 218)}


def test_constants_match_the_source():
    src = open(os.path.join(CSRC, "fmx_pairs.hip")).read()
    assert re.search(r"constexpr int FCP_UNR = %d;" % UNR, src)
    assert re.search(r"return t == 4 \|\| t == 8 \? t : %d;" % TILES[0], src)
    design = open(os.path.join(os.path.dirname(CSRC), "..", "DESIGN.md")).read()
    sec = design[design.index("4.2f"):]
    for t, (narrow, wide) in VGPR.items():
        assert re.search(r"T = %d[^\n]*\b%d\b[^\n]*\b%d\b" % (t, narrow, wide), sec), (t, narrow, wide)


def test_sweep_kernels(tmp_path_factory):
    text = isa(tmp_path_factory, "fmx_pairs")
    ks = kernels(text, "fcp_sweep_kernel")
    assert len(ks) == len(WIDTHS) * len(TILES)   # KH = 2 ... 64 x T = 4, 8
    for name, (body, meta) in ks.items():
        assert meta["private_seg_size"] == 0, f"{name}: scratch in the sweep kernel"
        assert meta["num_agpr"] == 0, (name, meta)
        assert "scratch_" not in body and "s_swappc" not in body
    for t in TILES:
        for kh in WIDTHS:
            (name, (body, meta)), = kernels(text, "fcp_sweep_kernelILi%dELi%dEE" % (kh, t)).items()
            assert meta["num_vgpr"] <= VGPR[t][1 if kh == 64 else 0], (name, meta)
            # no factor has a branch of its own
            assert len(re.findall(r"s_cbranch", body)) < UNR * t, name
            # the two products and the count of every (SNP, row cluster) are selects
            assert len(re.findall(r"v_cndmask", body)) >= 2 * UNR * t, name
        (name, (body, meta)), = kernels(text, "fcp_sweep_kernelILi64ELi%dEE" % t).items()
        # 64 partner lanes: the three diagonal values and the membership word of every (SNP, row cluster) of a loop step come
        # through scalar loads, and so do af and the partner block's membership word of every SNP ...
        assert len(re.findall(r"s_load_dwordx2", body)) >= (3 + 1) * UNR * t + 2 * UNR, name
        # ... the partner rows through vector loads, all of a step side by side
        assert len(re.findall(r"global_load_dwordx[24]", body)) >= UNR, name
    for pat in ("fcp_join_kernel", "fcp_member_kernel", "fcp_pack_kernel"):
        (name, (body, meta)), = kernels(text, pat).items()
        assert meta["private_seg_size"] == 0 and "scratch_" not in body
