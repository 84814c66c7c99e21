"""ISA facts of demux_ambient_fit.hip, from the code object's metadata only (no GPU needed, no instruction is inspected), in
the manner of test_isa_demux_alpha_fit.py: the unit holds the seven instantiations of amb_fit_kernel and nothing else, and
none of them uses scratch with the grid's NA x 9 products and the nine of a pass (three shares' a_l, or a, a', a'' of one
share) in registers."""
import re

from test_isa import isa, kernels


def test_the_fit_kernels_use_no_scratch(tmp_path_factory):
    text = isa(tmp_path_factory, "demux_ambient_fit")
    ks = kernels(text, "amb_fit_kernel")
    assert len(ks) == 7
    assert set(kernels(text, "")) == set(ks)  # every kernel of the unit is one of them
    seen = set()
    for name, (_body, meta) in sorted(ks.items()):
        na = int(re.search(r"amb_fit_kernelILi(\d+)E", name).group(1))
        seen.add(na)
        print(na, {k: meta.get(k) for k in ("num_vgpr", "num_agpr", "numbered_sgpr", "private_seg_size")})
        assert meta["private_seg_size"] == 0, f"{name}: scratch"
    assert seen == {2, 3, 4, 6, 8, 12, 16}
