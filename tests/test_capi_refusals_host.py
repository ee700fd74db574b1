"""Every refusal of the sml_host_* entry points, held to the recording tests/golden/g19_capi_refusals.json ("host"): the return
code and the FULL sml_last_error() text of each case of tests/_refusal_cases.py, and 0 for each valid call.  The recording was
made from the library as it was before the C API was split into capi.hip and capi_ops.hip; it is not regenerated.

Coverage, checked against that earlier source: every string literal that ivf_search_refusal, ivf_centroids_refusal, gram_refusal,
als_refusal, cooc_refusal, knn_refusal (with knn_overlap), graph_refusal, deep_refusal, rerank_refusal, neg_sampler_refusal,
neg_sets_overlap's caller and kNegSetsArgs can return is the text of at least one host case -- except the ones no host form can
reach, because the host forms pass device = false, max_workgroups = 0, path = 0, slices = 0 and no scratch:
  "scratch and gram must be 16-byte aligned" (gram_refusal), "gram must be 16-byte aligned" (als_refusal), "scratch must be 256-byte
  aligned" (cooc / knn / graph_refusal) and "src and out must be 16-byte aligned" (graph_refusal): test_capi_refusals_gpu.py;
  "bad argument (max_workgroups >= 0)" (als_refusal, rerank_refusal) and "bad argument (0 <= slices <= 256)" (deep_refusal):
  test_capi_refusals_gpu.py for the first and the last, the rerank one by test_rerank_gpu.py;
  "bad argument (max_workgroups >= 0, path 0 / 1 / 2)" (cooc / knn / graph_refusal): max_workgroups through
  test_capi_refusals_gpu.py, path through test_knn_gpu.py and test_graph_gpu.py.
"no walk for this (d, elem_bytes) pair" is unreachable by construction: the refusal functions ask sml_*_supports first."""
import _refusal_cases as R


def test_host_refusals_equal_the_recording():
    from sml_amd import _lib
    got = R.run(_lib.load(), R.host_cases())
    for c in R.host_cases():
        assert got[c["fn"] + ":valid"] == [0, ""], c["fn"]
    want = R.recorded("host")
    assert len(want) > 300 and sum(1 for rc, _ in want.values() if rc != 0) > 250
    R.assert_same(got, want)
