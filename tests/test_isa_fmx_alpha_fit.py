"""ISA facts of fmx_alpha_fit.hip, from the code object's metadata only (no GPU needed, no instruction is inspected), in
the manner of test_isa_fmx_ambient_fit.py: the unit holds one kernel, fma_fit_kernel; it uses no scratch and no AGPRs, and
its VGPR count is the one DESIGN 4.2l quotes, within 168 (three waves per SIMD) with its nine entry likelihoods and the
eighteen products of a pass (three shares' six elements, or a, a', a'' of the six) in registers."""
import os
import re

from test_isa import ROOT, isa, kernels


def test_the_fit_kernel_uses_no_scratch_no_agprs_and_the_vgprs_design_quotes(tmp_path_factory):
    text = isa(tmp_path_factory, "fmx_alpha_fit")
    ks = kernels(text, "fma_fit_kernel")
    assert len(ks) == 1
    assert set(kernels(text, "")) == set(ks)  # every kernel of the unit is this one
    quoted = int(re.search(r"fma_fit_kernel: (\d+) VGPRs", open(os.path.join(ROOT, "DESIGN.md")).read()).group(1))
    for name, (_body, meta) in ks.items():
        print(name, {k: meta.get(k) for k in ("num_vgpr", "num_agpr", "numbered_sgpr", "private_seg_size")})
        assert meta["private_seg_size"] == 0, f"{name}: scratch"
        assert meta["num_agpr"] == 0, (name, meta)
        assert meta["num_vgpr"] == quoted and quoted <= 168, (name, meta, quoted)
