"""ISA facts of demux_ambient.hip, from the code object's metadata only (no GPU needed, no instruction is inspected), in the
manner of test_isa_fmx_ambient.py: which kernels the unit holds and how many of each, no scratch anywhere, and the sweeps
of muxgl_demux_ambient -- ambient_table.hpp's kernel under this unit's UNR rule -- keep the loads of a renormalisation
block in flight in registers: no AGPRs, no LDS, and the register counts the build had before the sweep moved to the shared
header."""
import re

from test_isa import isa, kernels

# VGPRs of the sweeps, read off the build of the commit before ambient_table.hpp (hipcc of ROCm 7, gfx950): four rhos of
# four entries per lane take 134 below 64 columns (widths 2 .. 32: three waves per SIMD), every other instantiation fits
# 128 (four waves per SIMD; the largest are 128 at <VH = 1, CH = 4> and 100 elsewhere)
SWEEP_VGPR_WIDE = 134
SWEEP_VGPR = 128


def lds_bytes(text, name):
    """the kernel descriptor's static LDS size"""
    m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n.*?\.amdhsa_group_segment_fixed_size (\d+)", text, re.S)
    assert m, name
    return int(m.group(1))


def test_kernels_of_the_unit_and_their_registers(tmp_path_factory):
    text = isa(tmp_path_factory, "demux_ambient")
    ks = kernels(text, "ambient_sweep_kernel")
    assert len(ks) == 28  # VH = 1, 2, 4, 8, 16, 32, 64 x CH = 1, 2, 3, 4
    shapes = set()
    for name, (_body, meta) in ks.items():
        assert "amb_sweep" in name, name  # this unit's UNR rule
        vh, ch = map(int, re.search(r"ELi(\d+)ELi(\d+)EE", name).groups())
        shapes.add((vh, ch))
        assert meta["private_seg_size"] == 0, f"{name}: scratch in a sweep kernel"
        assert meta["num_agpr"] == 0, (name, meta)
        assert meta["num_vgpr"] <= (SWEEP_VGPR_WIDE if ch == 4 and 2 <= vh <= 32 else SWEEP_VGPR), (name, meta)
        assert lds_bytes(text, name) == 0, name
    assert shapes == {(vh, ch) for vh in (1, 2, 4, 8, 16, 32, 64) for ch in (1, 2, 3, 4)}
    wk = kernels(text, "amb_weight_kernel")
    # NA = 2, 3, 4 x RC = 4, 8, 16; NA = 6, 8 x RC = 4, 8; NA = 12, 16 x RC = 4
    assert len(wk) == 15
    ek = kernels(text, "ambient_emit_kernel")
    assert len(ek) == 1
    ck = kernels(text, "amb_count_kernel")
    assert len(ck) == 1
    seen = {**ks, **wk, **ek, **ck}
    assert set(kernels(text, "")) == set(seen)  # every kernel of the unit is one of these
    for name, (_body, meta) in seen.items():
        assert meta["private_seg_size"] == 0, f"{name}: scratch"
        print(name, {k: meta.get(k) for k in ("num_vgpr", "num_agpr", "numbered_sgpr", "private_seg_size", "group_segment_fixed_size")})
