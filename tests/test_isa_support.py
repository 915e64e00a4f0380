"""What the compiler makes of igd_sets_support (engine/support_dev.hpp); no GPU needed, hipcc cross-compiles gfx950.
The LDS form keeps the waves' file bitmaps and the workgroup's counters in LDS: the bitmap must be reached with an LDS
atomic OR that returns the old word (ds_or_rtn_b32) and the counters with ds_add_u32 -- not with flat atomics that resolve
to LDS at run time -- and the kernel must not spill.  The wide form (more files than the LDS form takes) keeps its bitmaps
in global memory: a returning global atomic OR, and no LDS atomics at all."""
from test_isa_guards import body, field, isa  # noqa: F401  (isa: the session's device assembly)

SIG = "EEv6DbViewPKiS2_S2_PK8SetSliceiiiPyS6_Pj"
LDS_FORMS = ["_Z16igd_sets_supportILb0ELb1" + SIG, "_Z16igd_sets_supportILb1ELb1" + SIG]
WIDE_FORMS = ["_Z16igd_sets_supportILb0ELb0" + SIG, "_Z16igd_sets_supportILb1ELb0" + SIG]


def test_lds_form_reaches_its_bitmap_with_a_returning_atomic_of_the_lds(isa):
    for sym in LDS_FORMS:
        code, desc = body(isa, sym)
        assert field(desc, "private_segment_fixed_size") == 0, sym + " uses scratch (spills)"
        assert "scratch_" not in code
        assert "ds_or_rtn_b32" in code, sym + ": no returning LDS atomic OR on the bitmap"
        assert "ds_add_u32" in code, sym + ": no LDS atomic add on the workgroup's counters"
        assert "flat_atomic" not in code, sym + ": a flat atomic (LDS reached through a generic pointer?)"
        assert "global_atomic_or" not in code
        assert field(desc, "next_free_vgpr") <= 64, sym + ": fewer than 8 waves per SIMD"


def test_wide_form_keeps_its_bitmap_in_global_memory(isa):
    for sym in WIDE_FORMS:
        code, desc = body(isa, sym)
        assert field(desc, "private_segment_fixed_size") == 0, sym + " uses scratch (spills)"
        assert "global_atomic_or" in code and "flat_atomic" not in code
        assert "ds_or" not in code and "ds_add" not in code
