"""igd_amd -- MI355X-native overlap search for IGD databases (databio/IGD's `igd search` hot
path), behind the reference's own C ABI.  See DESIGN.md / INTEGRATION.md."""
from ._native import NativeMissing, build  # noqa: F401

__all__ = ["Database", "NativeMissing", "build", "fisher_host", "rank_host", "restrict_host", "enrich_restricted_host",
           "cooccur_host", "bitrows_gram_host", "jaccard", "perm_summary", "permute_regions_host", "permute_host", "MinOverlap",
           "search_host", "support_host", "nearest_host", "nearest_sets_host", "nearest_summary", "NearestSets", "permute_nearest_host",
           "perm_nearest_summary", "PermutationNearest", "map_host", "map_sets_host", "map_summary", "MapSets",
           "nearest_signed_host", "nearest_hist_host", "NearestHist", "NEAREST_NO_RECORD",
           "flanks_host", "flank_reldist_host", "reldist_summary", "FlankReldist", "FLANK_EDGES", "FLANK_MIDPOINTS", "FLANK_MAX_BINS",
           "merge_host", "dataset_bp_host", "jaccard_host", "jaccard_summary", "JaccardSets", "MERGE_MAX_GAP",
           "permute_bp_host", "perm_bp_summary", "PermutationBp", "Workspace", "build_workspace",
           "DatasetGroups", "build_groups", "read_groups_file", "GROUP_MAX", "ShiftSupport", "shift_offsets", "local_zscore",
           "perm_map_summary", "PermutationMap"]
# (igd_amd.group_support_host resolves below like the other host routes; it is not in __all__, whose `_host` names with regions are
# the table of tests/test_database_args_host.py; so do igd_amd.shift_support_host, igd_amd.shift_regions_host
# igd_amd.resample_regions_host and igd_amd.permute_map_host)
# `from igd_amd import igd_py as iGD; iGD.igd_py()` mirrors the reference's `import igd_py as iGD`


def __getattr__(name):
    if name == "Database":
        from .database import Database
        return Database
    if name == "fisher_host":
        from .database import fisher_host
        return fisher_host
    if name == "rank_host":
        from .database import rank_host
        return rank_host
    if name == "restrict_host":
        from .database import restrict_host
        return restrict_host
    if name == "enrich_restricted_host":
        from .database import enrich_restricted_host
        return enrich_restricted_host
    if name in ("cooccur_host", "bitrows_gram_host", "jaccard", "perm_summary", "permute_regions_host", "permute_host", "MinOverlap",
                "search_host", "support_host", "nearest_host", "nearest_sets_host", "nearest_summary", "NearestSets", "permute_nearest_host",
                "perm_nearest_summary", "PermutationNearest", "map_host", "map_sets_host", "map_summary", "MapSets",
                "nearest_signed_host", "nearest_hist_host", "NearestHist", "NEAREST_NO_RECORD",
                "flanks_host", "flank_reldist_host", "reldist_summary", "FlankReldist", "FLANK_EDGES", "FLANK_MIDPOINTS", "FLANK_MAX_BINS",
                "merge_host", "dataset_bp_host", "jaccard_host", "jaccard_summary", "JaccardSets", "MERGE_MAX_GAP",
                "permute_bp_host", "perm_bp_summary", "PermutationBp", "Workspace", "build_workspace",
           "DatasetGroups", "build_groups", "read_groups_file", "group_support_host", "GROUP_MAX",
                "ShiftSupport", "shift_offsets", "local_zscore", "shift_support_host", "shift_regions_host",
                "resample_regions_host", "permute_map_host", "perm_map_summary", "PermutationMap"):
        from . import database
        return getattr(database, name)
    raise AttributeError(name)
