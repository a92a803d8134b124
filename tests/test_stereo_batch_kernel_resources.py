"""CPU: batching the stereo matchers re-indexes the existing kernels (blockIdx.z = the pair) and adds
none.  From the compiler's remarks of the build: the matcher's kernels are exactly the set the
one-pair path had, every one of them without scratch memory and spills, and any kernel beyond that
set -- a new one -- would have to stay within the wave budget of its one-pair sibling
(tests/test_sgbm_abi.py, tests/test_bm_abi.py: eight waves per SIMD for the SGBM chains, four for
k_bm_match)."""
import re

from test_kernel_resources import _kernels

ONE_PAIR = {"k_sgbm_hsum", "k_sgbm_vsum", "k_sgbm_path", "k_sgbm_lrcheck", "k_sgbm_median",
            "k_sgbm_uf_init", "k_sgbm_uf_union", "k_sgbm_uf_count", "k_sgbm_final", "k_bm_prefilter",
            "k_bm_match", "k_densify_count", "k_densify_scan", "k_densify_emit", "k_densify_append_scan",
            "k_densify_append_emit", "k_rectify"}
# what a new batch kernel is held to: the occupancy floor of the one-pair kernel it stands beside
SIBLING_WAVES = {"k_sgbm_path": 8, "k_bm_match": 3}


def _stereo_kernels():
    out = {}
    for mangled, v in _kernels().items():
        m = re.match(r"^_ZN5amhip\d+(k_(?:sgbm|bm|densify|rectify|seq|stereo)\w*?)(?:I[\w]*?E{1,3}v|E)", mangled)
        if m:
            out.setdefault(m.group(1), []).append((mangled, v))
    return out


def test_the_batch_adds_no_kernel_and_none_uses_scratch():
    ks = _stereo_kernels()
    assert {"k_sgbm_path", "k_bm_match", "k_sgbm_final", "k_sgbm_uf_union"} <= set(ks), sorted(ks)
    for name, versions in ks.items():
        for mangled, v in versions:
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (mangled, v)
    new = set(ks) - ONE_PAIR
    for name in new:   # (none today; a new one answers to its sibling's budget)
        sibling = next((s for s in SIBLING_WAVES if name.startswith(s)), "k_sgbm_path")
        for mangled, v in ks[name]:
            assert v["Occupancy"] >= SIBLING_WAVES[sibling], (mangled, v)
    assert len(ks["k_sgbm_path"]) == 12 and len(ks["k_bm_match"]) == 16


def test_re_indexed_kernels_keep_their_occupancy():
    ks = _stereo_kernels()
    for mangled, v in ks["k_sgbm_path"]:
        assert v["Occupancy"] >= 8, (mangled, v)
    for name in ("k_sgbm_vsum", "k_sgbm_lrcheck", "k_sgbm_median", "k_sgbm_uf_init", "k_sgbm_uf_union",
                 "k_sgbm_uf_count", "k_sgbm_final", "k_bm_prefilter"):
        (mangled, v), = ks[name]
        assert v["Occupancy"] >= 8, (mangled, v)
    for mangled, v in ks["k_bm_match"]:
        assert v["Occupancy"] >= 3, (mangled, v)
