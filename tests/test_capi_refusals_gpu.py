"""The refusals only a call with a context reaches, held to the recording tests/golden/g19_capi_refusals.json ("gpu", made on an
MI355X from the library as it was before the C API was split): catalogue_ok through sml_full_rank, sml_topk_items and
sml_user_rank in their plain, _f16, _filtered and _adjusted forms; sml_topk_candidates; the alignment checks of sml_ivf_search,
sml_topk_deep, sml_gram, sml_als_solve, sml_cooc_topk, sml_knn_topk and sml_graph_propagate; sml_iset_build and sml_iset_union;
sml_item_adjust_* and sml_item_filter_from_ids; sml_user_metrics.  Return code and full sml_last_error() text per case.

Every refused case here would be harmless if the library accepted it (tests/_refusal_cases.py says how): this test is no way to
start a kernel on bad memory.  Null-argument refusals are the host forms' and the older GPU tests' business."""
import pytest

import _refusal_cases as R


@pytest.mark.gpu
def test_gpu_refusals_equal_the_recording():
    from sml_amd import _lib
    lib = _lib.load()
    with R.Contexts(lib) as ctx_of:
        got = R.run(lib, R.gpu_cases(), "cuda:0", ctx_of)
    for c in R.gpu_cases():
        assert got[c["fn"] + ":valid"] == [0, ""], (c["fn"], got[c["fn"] + ":valid"])
    want = R.recorded("gpu")
    assert len(want) > 100 and sum(1 for rc, _ in want.values() if rc != 0) > 80
    R.assert_same(got, want)
