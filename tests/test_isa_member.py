"""What the compiler makes of igd_member_rows (engine/member_dev.hpp); no GPU needed, hipcc cross-compiles gfx950.
The LDS form keeps the waves' file bitmaps in LDS and must reach them with an LDS atomic OR -- not with flat atomics that
resolve to LDS at run time -- without spilling and within 64 VGPRs (8 waves per SIMD).  The wide form ORs straight into the
output rows in global memory and uses no LDS atomic OR at all."""
from test_isa_guards import body, field, isa  # noqa: F401  (isa: the session's device assembly)

LDS_FORMS = ["_Z15igd_member_rowsILb0ELb1EE", "_Z15igd_member_rowsILb1ELb1EE"]
WIDE_FORMS = ["_Z15igd_member_rowsILb0ELb0EE", "_Z15igd_member_rowsILb1ELb0EE"]


def test_lds_form_ors_into_its_bitmap_with_an_atomic_of_the_lds(isa):
    for sym in LDS_FORMS:
        code, desc = body(isa, sym)
        assert field(desc, "private_segment_fixed_size") == 0, sym + " uses a private segment (spills)"
        assert field(desc, "next_free_vgpr") <= 64, sym + ": fewer than 8 waves per SIMD"
        assert "ds_or" in code, sym + ": no LDS atomic OR on the bitmap"
        assert "flat_atomic" not in code, sym + ": a flat atomic (LDS reached through a generic pointer?)"


def test_wide_form_ors_into_the_rows_in_global_memory(isa):
    for sym in WIDE_FORMS:
        code, desc = body(isa, sym)
        assert field(desc, "private_segment_fixed_size") == 0, sym + " uses a private segment (spills)"
        assert field(desc, "next_free_vgpr") <= 64, sym + ": fewer than 8 waves per SIMD"
        assert "global_atomic_or" in code and "flat_atomic" not in code
        assert "ds_or" not in code and "ds_add" not in code, sym + ": an LDS atomic in the wide form"
