"""ISA facts of fmx_unknown.hip, from the code object's metadata only (no GPU needed), in the manner of
test_isa_fmx_singlets.py: the sweeps of muxgl_fmx_unknown keep the loads of a renormalisation block in flight in
registers -- no scratch, no AGPRs, no LDS, four waves per SIMD -- in every instantiation: the cluster sweep once per
width of a cluster block (1 .. 64) and the sweep of the two per-cell scalars."""
import os
import re

from test_isa import CSRC, isa, kernels

UNR = 8  # FUN_UNR: entries per lane between two renormalisations


def test_constant_matches_the_source():
    src = open(os.path.join(CSRC, "fmx_unknown.hip")).read()
    assert re.search(r"constexpr int FUN_UNR = %d;" % UNR, src)


def test_sweep_kernels_use_no_scratch_no_agprs_no_lds(tmp_path_factory):
    text = isa(tmp_path_factory, "fmx_unknown")
    ks = kernels(text, "fun_sweep_kernel")
    assert len(ks) == 7  # KH = 1, 2, 4, 8, 16, 32, 64
    sc = kernels(text, "fun_scalar_kernel")
    assert len(sc) == 1
    for name, (_body, meta) in {**ks, **sc}.items():
        assert meta["private_seg_size"] == 0, f"{name}: scratch in a sweep kernel"
        assert meta["num_agpr"] == 0, (name, meta)
        assert meta["num_vgpr"] <= 128, (name, meta)  # four waves per SIMD at least
        assert meta.get("group_segment_fixed_size", 0) == 0, (name, meta)
    for pattern in ("fun_prior_kernel", "fun_weight_kernel", "fun_split_kernel", "table_join_kernel"):
        ks = kernels(text, pattern)
        assert len(ks) == 1, pattern
        for name, (_body, meta) in ks.items():
            assert meta["private_seg_size"] == 0 and meta.get("group_segment_fixed_size", 0) == 0, (name, meta)
