"""The argument refusals of the stateless C entry points, as data: per entry point one valid call on tiny arrays and a list of
single-argument mutations of it.  tests/golden/make_golden_refusals.py records what a built library answers to each (return code
and the full sml_last_error() text) in tests/golden/g19_capi_refusals.json; test_capi_refusals_host.py and
test_capi_refusals_gpu.py hold every later build to that recording, byte for byte.

Sizes: d = 32 fp32, 40 items, 6 users, n = 3, k = 4; 5 lists with nprobe 2 where lists apply.

Every array sits at the start of a zeroed, 256-byte aligned block of at least BACK bytes, so a mutated pointer -- another
argument's array (an overlap) or the argument's own array a few bytes in (a misalignment) -- always points into memory of the
test's own that is large enough for whatever the call would read or write there.  The GPU cases keep to that rule strictly (no
null or foreign pointer, and a bad scalar is one that the launcher itself refuses or that leaves the kernels nothing to walk):
they are refused before any launch, and would be harmless if they were not.  Per kind of scalar: elem_bytes 3 and a d = 128
context on fp32 tables are pairs the launchers refuse (hipErrorInvalidValue, nothing started; the blocks would hold d = 128 rows
anyway); n_item 0 leaves the slice walks no tile and the per-item launches an empty grid; n_cols 1 leaves sml_full_rank no
candidate column and sml_iset_build reads column 1 of the next row, inside its block; a negative cand_cols is an empty candidate
list (cand_stride and cand_first stay valid, so no address before the block is formed); a negative max_workgroups or slices is
taken as 0 by every launcher; n_user 0, n_k 0, invert 2 and a 0 in ks start nothing that indexes memory by them."""
import ctypes

import numpy as np

D, N_ITEM, N_USER, N, K, N_LIST, NPROBE = 32, 40, 6, 3, 4, 5, 2
BACK = 1 << 15            # bytes behind every array, at least: the largest write a wrongly accepted overlap could make is 8 KiB
                          # (a Gram matrix), the largest read 20 KiB (the 40-row table taken as d = 128 fp32 rows by a Ctx(128) case)
SCRATCH = 1 << 20         # one scratch block serves every device call (asserted against the library's own *_scratch_bytes)


class At:
    """The address of argument `name`'s array plus `off` bytes."""
    def __init__(self, name, off=0):
        self.name, self.off = name, off


class Ctx:
    """A context of embedding width d (GPU cases)."""
    def __init__(self, d=D):
        self.d = d


class Host:
    """An array the library reads on the host even in a device call (sml_user_metrics' ks)."""
    def __init__(self, arr):
        self.arr = arr


class Mem:
    """Places arrays: in host memory (device None) or on a GPU through torch."""
    def __init__(self, device=None):
        self.device, self.keep = device, []

    def put(self, arr, host=False):
        raw = np.frombuffer(np.ascontiguousarray(arr).tobytes(), np.uint8)
        nbytes = max(raw.size, BACK)
        if self.device is None or host:
            block = np.zeros(nbytes + 256, np.uint8)
            off = (-block.ctypes.data) % 256
            block[off:off + raw.size] = raw
            self.keep.append(block)
            return block.ctypes.data + off
        import torch
        t = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        t[:raw.size] = torch.from_numpy(raw.copy()).to(self.device)
        assert t.data_ptr() % 256 == 0
        self.keep.append(t)
        return t.data_ptr()


def _f32(shape, seed):
    return ((np.arange(int(np.prod(shape)), dtype=np.float32) * (0.37 + seed) % 1.0) - 0.5).reshape(shape).astype(np.float32)


def _data():
    """The shared inputs: user u holds the items (7u + 3j) % 40, j < 5; item i is in list i % 5."""
    z = {}
    sets = [sorted({(7 * u + 3 * j) % N_ITEM for j in range(5)}) for u in range(N_USER)]
    z["u_off"] = np.cumsum([0] + [len(s) for s in sets]).astype(np.int64)
    z["u_items"] = np.array([i for s in sets for i in s], np.int32)
    by_item = [[u for u in range(N_USER) if i in sets[u]] for i in range(N_ITEM)]
    z["i_off"] = np.cumsum([0] + [len(s) for s in by_item]).astype(np.int64)
    z["i_users"] = np.array([u for s in by_item for u in s], np.int32)
    z["w_user"], z["w_item"] = _f32((N_USER, D), 0.0), _f32((N_ITEM, D), 0.1)
    z["w_user_h"], z["w_item_h"] = z["w_user"].astype(np.float16), z["w_item"].astype(np.float16)
    z["users"] = np.array([0, 2, 4], np.int64)
    lists = [[i for i in range(N_ITEM) if i % N_LIST == c] for c in range(N_LIST)]
    z["list_off"] = np.cumsum([0] + [len(s) for s in lists]).astype(np.int64)
    z["list_items"] = np.array([i for s in lists for i in s], np.int32)
    z["probes"] = np.array([[0, 1], [2, 3], [4, 0]], np.int32)
    z["allow"] = np.full(2, 0xffffffff, np.uint32)                 # 64 padded items
    z["adj"] = np.concatenate([np.ones(64, np.float32), np.zeros(64, np.float32)])
    z["cent"] = _f32((N_LIST, D), 0.2)
    z["gram"] = np.eye(D, dtype=np.float64)
    z["norm"] = np.ones(N_ITEM, np.float64)
    z["nbr_items"] = (np.arange(N_ITEM * 4, dtype=np.int32).reshape(N_ITEM, 4) * 7 + 1) % N_ITEM
    z["nbr_sims"] = np.tile(np.array([0.9, 0.7, 0.5, 0.3], np.float32), (N_ITEM, 1))
    z["a"], z["b"] = np.ones(N_USER, np.float32), np.ones(N_ITEM, np.float32)
    z["pool_items"] = np.array([[(5 * x + 3 * c) % N_ITEM for c in range(8)] for x in range(N)], np.int32)
    z["pool_rel"] = np.tile(np.linspace(1.0, 0.2, 8, dtype=np.float32), (N, 1))
    z["nrm"] = np.ones(N_ITEM, np.float32)
    # a stream of 15 rows: row g is (g % 6, 3g % 40), every item new; the call serves rows 12 .. 14
    stream = np.array([[g % N_USER, (3 * g) % N_ITEM] for g in range(15)], np.int64)
    z["ns_rows"], z["ns_ncat"] = stream[12:].copy(), np.array([13, 14, 15], np.int32)
    z["ns_order"] = stream[:, 1].astype(np.int32)
    pairs = sorted((int(u), int(i), g) for g, (u, i) in enumerate(stream))
    z["ns_hoff"] = np.cumsum([0] + [sum(1 for p in pairs if p[0] == u) for u in range(N_USER)]).astype(np.int64)
    z["ns_hitems"] = np.array([p[1] for p in pairs], np.int32)
    z["ns_hsince"] = np.array([p[2] for p in pairs], np.int32)
    z["item_all"] = np.arange(N_ITEM, dtype=np.int64)
    z["u_items64"] = z["u_items"].astype(np.int64)
    z["cand"] = np.array([1, 2, 5, 6, 9, 11, 13, 17], np.int64)
    z["pairs"] = np.sort(np.array([u * 1000 + i for u in range(N_USER) for i in sets[u]], np.int64))
    z["ui"] = np.array([[u, i] for u in range(N_USER) for i in sets[u]], np.int64)
    z["order3"] = np.array([4, 0, 9], np.int64)
    z["mat"] = np.arange(30 * 3, dtype=np.int64).reshape(30, 3)
    return z


Z = _data()


def _i32(*shape):
    return np.zeros(shape, np.int32)


def _out_f32(*shape):
    return np.zeros(shape, np.float32)


def _case(fn, args, muts):
    return {"fn": fn, "args": args, "muts": muts}


def host_cases():
    z = Z
    cases = []
    cat = [("w_user", z["w_user"]), ("w_item", z["w_item"]), ("elem_bytes", 4), ("d", D), ("n_item", N_ITEM), ("users", z["users"]), ("n", N)]
    tail = [("seen_off", z["u_off"]), ("seen_items", z["u_items"]), ("allow", z["allow"]), ("adj", z["adj"])]
    outs = [("items", _i32(N, K)), ("scores", _out_f32(N, K)), ("n_elig", _i32(N))]
    shared = [("elem_bytes_3", {"elem_bytes": 3}), ("d_48", {"d": 48}), ("d_128_fp32", {"d": 128}), ("n_item_0", {"n_item": 0}),
              ("n_item_2^31", {"n_item": 1 << 31}), ("n_negative", {"n": -1}), ("k_0", {"k": 0}), ("seen_off_alone", {"seen_items": None}),
              ("seen_items_alone", {"seen_off": None}), ("n_0", {"n": 0}), ("w_user_null", {"w_user": None}), ("w_item_null", {"w_item": None}),
              ("users_null", {"users": None}), ("items_null", {"items": None}), ("scores_null", {"scores": None}),
              ("n_elig_null", {"n_elig": None}), ("no_seen_allow_adj", {"seen_off": None, "seen_items": None, "allow": None, "adj": None}),
              ("items_on_users", {"items": At("users")}), ("items_on_w_user", {"items": At("w_user")}), ("scores_on_w_item", {"scores": At("w_item", 64)}),
              ("n_elig_on_seen_off", {"n_elig": At("seen_off")}), ("items_on_seen_items", {"items": At("seen_items")}),
              ("scores_on_allow", {"scores": At("allow")}), ("n_elig_on_adj", {"n_elig": At("adj", 500)}),
              ("items_behind_users", {"items": At("users", 8 * N)}),
              ("scores_on_items", {"scores": At("items")}), ("n_elig_on_items", {"n_elig": At("items", 44)}),
              ("n_elig_on_scores", {"n_elig": At("scores")}), ("n_elig_behind_items", {"n_elig": At("items", 4 * N * K)})]
    cases.append(_case("sml_host_ivf_search",
                       cat + [("list_off", z["list_off"]), ("list_items", z["list_items"]), ("n_list", N_LIST), ("probes", z["probes"]),
                              ("nprobe", NPROBE), ("k", K)] + tail + outs,
                       shared + [("nprobe_0", {"nprobe": 0}), ("nprobe_129", {"nprobe": 129}), ("n_list_0", {"n_list": 0}), ("k_129", {"k": 129}),
                                 ("list_off_null", {"list_off": None}), ("list_items_null", {"list_items": None}), ("probes_null", {"probes": None}),
                                 ("items_on_list_off", {"items": At("list_off")}), ("scores_on_list_items", {"scores": At("list_items")}),
                                 ("n_elig_on_probes", {"n_elig": At("probes", 20)}), ("fp16", {"w_user": z["w_user_h"], "w_item": z["w_item_h"], "elem_bytes": 2})]))
    cases.append(_case("sml_host_topk_items", cat + [("k", K)] + tail + outs,
                       shared + [("k_1025", {"k": 1025}), ("n_2^31", {"n": 1 << 31}), ("n_item_negative", {"n_item": -5})]))
    cases.append(_case("sml_host_ivf_centroids",
                       [("w_item", z["w_item"]), ("elem_bytes", 4), ("d", D), ("n_item", N_ITEM), ("list_off", z["list_off"]),
                        ("list_items", z["list_items"]), ("n_list", N_LIST), ("cin", z["cent"]), ("cout", z["cent"] * 0)],
                       [("elem_bytes_8", {"elem_bytes": 8}), ("d_128_fp32", {"d": 128}), ("n_item_0", {"n_item": 0}), ("n_item_2^31", {"n_item": 1 << 31}),
                        ("n_list_0", {"n_list": 0}), ("w_item_null", {"w_item": None}), ("list_off_null", {"list_off": None}),
                        ("list_items_null", {"list_items": None}), ("cin_null", {"cin": None}), ("cout_null", {"cout": None}),
                        ("in_place", {"cout": At("cin")}), ("cout_one_row_into_cin", {"cout": At("cin", 4 * D)}),
                        ("cout_behind_cin", {"cout": At("cin", 4 * D * N_LIST)}), ("cout_on_w_item", {"cout": At("w_item")}),
                        ("cout_on_list_off", {"cout": At("list_off", 40)}), ("cout_on_list_items", {"cout": At("list_items", 156)})]))
    cases.append(_case("sml_host_gram", [("w", z["w_item"]), ("elem_bytes", 4), ("d", D), ("n_rows", N_ITEM), ("gram", np.zeros((D, D)))],
                       [("elem_bytes_3", {"elem_bytes": 3}), ("d_128", {"d": 128}), ("n_rows_0", {"n_rows": 0}), ("n_rows_2^31", {"n_rows": 1 << 31}),
                        ("w_null", {"w": None}), ("gram_null", {"gram": None}), ("gram_on_w", {"gram": At("w")}),
                        ("gram_on_w_end", {"gram": At("w", 4 * D * N_ITEM - 8)}), ("gram_behind_w", {"gram": At("w", 4 * D * N_ITEM)})]))
    cases.append(_case("sml_host_als_solve",
                       [("w_other", z["w_item"]), ("elem_bytes", 4), ("d", D), ("n_other", N_ITEM), ("gram", z["gram"]), ("alpha0", 0.5), ("reg", 0.1),
                        ("set_off", z["u_off"]), ("set_items", z["u_items"]), ("rows", z["users"]), ("n", N), ("w_out", _out_f32(N_USER, D)),
                        ("n_out", N_USER), ("status", _i32(N))],
                       [("elem_bytes_3", {"elem_bytes": 3}), ("d_128", {"d": 128}), ("reg_negative", {"reg": -1.0}), ("alpha0_nan", {"alpha0": float("nan")}),
                        ("n_other_0", {"n_other": 0}), ("n_out_0", {"n_out": 0}), ("n_out_2^31", {"n_out": 1 << 31}), ("n_negative", {"n": -1}),
                        ("n_2^31", {"n": 1 << 31}), ("set_off_alone", {"set_items": None}), ("set_items_alone", {"set_off": None}),
                        ("gram_null", {"gram": None}), ("gram_null_alpha0_0", {"gram": None, "alpha0": 0.0}), ("n_0", {"n": 0}),
                        ("w_other_null", {"w_other": None}), ("w_out_null", {"w_out": None}), ("status_null", {"status": None}),
                        ("w_out_on_w_other", {"w_out": At("w_other")}), ("w_out_on_gram", {"w_out": At("gram", 8000)}),
                        ("w_out_on_set_off", {"w_out": At("set_off")}), ("w_out_on_set_items", {"w_out": At("set_items")}),
                        ("w_out_on_rows", {"w_out": At("rows", 16)}), ("w_out_on_status", {"w_out": At("status")}),
                        ("status_on_w_out", {"status": At("w_out", 100)}), ("status_on_w_other", {"status": At("w_other")}),
                        ("status_on_gram", {"status": At("gram")}), ("status_on_set_off", {"status": At("set_off")}),
                        ("status_on_set_items", {"status": At("set_items")}), ("status_on_rows", {"status": At("rows")}),
                        ("status_on_set_items_2nd_entry", {"status": At("set_items", 4)}), ("no_rows_status_on_set_off_2nd_entry", {"rows": None, "status": At("set_off", 8)}),
                        ("status_behind_rows", {"status": At("rows", 8 * N)})]))
    def each_input(outs3, ins):          # every input once under one of the three list outputs, in turn
        return [("%s_on_%s" % (outs3[q % 3], name), {outs3[q % 3]: At(name)}) for q, name in enumerate(ins)]
    cooc = [("by_item_off", z["i_off"]), ("by_item_users", z["i_users"]), ("by_user_off", z["u_off"]), ("by_user_items", z["u_items"]),
            ("n_user", N_USER), ("n_item", N_ITEM), ("rows", z["users"]), ("n", N), ("norm_a", z["norm"]), ("norm_b", z["norm"].copy()),
            ("shrink", 1.0), ("min_co", 1), ("allow", z["allow"]), ("k", K), ("items", _i32(N, K)), ("sims", _out_f32(N, K)), ("n_elig", _i32(N))]
    cooc_in = ["by_item_off", "by_item_users", "by_user_off", "by_user_items", "rows", "norm_a", "norm_b", "allow"]
    cases.append(_case("sml_host_cooc_topk", cooc,
                       [("k_0", {"k": 0}), ("k_129", {"k": 129}), ("min_co_0", {"min_co": 0}), ("shrink_negative", {"shrink": -1.0}),
                        ("shrink_nan", {"shrink": float("nan")}), ("by_item_off_alone", {"by_item_users": None}), ("by_user_items_alone", {"by_user_off": None}),
                        ("norm_a_alone", {"norm_b": None}), ("n_item_0", {"n_item": 0}), ("n_user_2^31", {"n_user": 1 << 31}), ("n_negative", {"n": -1}),
                        ("n_0", {"n": 0}), ("items_null", {"items": None}), ("sims_null", {"sims": None}),
                        ("by_item_without_by_user", {"by_user_off": None, "by_user_items": None}), ("no_norms", {"norm_a": None, "norm_b": None}),
                        ("sims_on_items", {"sims": At("items")}), ("n_elig_on_items", {"n_elig": At("items", 4)}), ("n_elig_on_sims", {"n_elig": At("sims", 44)}),
                        ("n_elig_behind_sims", {"n_elig": At("sims", 4 * N * K)})]
                       + each_input(["items", "sims", "n_elig"], cooc_in)))
    knn = [("nbr_items", z["nbr_items"]), ("nbr_sims", z["nbr_sims"]), ("n_rows_nbr", N_ITEM), ("k_nbr", 4), ("n_item", N_ITEM), ("hist_off", z["u_off"]),
           ("hist_items", z["u_items"]), ("users", z["users"]), ("n", N), ("frac_bits", 16), ("seen_off", z["u_off"].copy()),
           ("seen_items", z["u_items"].copy()), ("allow", z["allow"]), ("k", K), ("items", _i32(N, K)), ("scores", _out_f32(N, K)), ("n_elig", _i32(N))]
    knn_in = ["nbr_items", "nbr_sims", "hist_off", "hist_items", "users", "seen_off", "seen_items", "allow"]
    cases.append(_case("sml_host_knn_topk", knn,
                       [("k_0", {"k": 0}), ("k_nbr_129", {"k_nbr": 129}), ("frac_bits_33", {"frac_bits": 33}), ("frac_bits_negative", {"frac_bits": -1}),
                        ("hist_off_alone", {"hist_items": None}), ("seen_items_alone", {"seen_off": None}), ("n_item_0", {"n_item": 0}),
                        ("n_rows_nbr_negative", {"n_rows_nbr": -1}), ("n_2^31", {"n": 1 << 31}), ("n_0", {"n": 0}), ("items_null", {"items": None}),
                        ("scores_null", {"scores": None}), ("nbr_items_null", {"nbr_items": None}), ("nbr_sims_null", {"nbr_sims": None}),
                        ("no_table", {"nbr_items": None, "nbr_sims": None, "n_rows_nbr": 0}), ("no_users", {"users": None}),
                        ("no_users_n_elig_on_hist_off_3rd_entry", {"users": None, "n_elig": At("hist_off", 16)}),
                        ("no_users_scores_on_seen_off_2nd_entry", {"users": None, "scores": At("seen_off", 8)}),
                        ("scores_on_items", {"scores": At("items", 47)}), ("n_elig_on_scores", {"n_elig": At("scores")}),
                        ("n_elig_on_items", {"n_elig": At("items")})]
                       + each_input(["items", "scores", "n_elig"], knn_in)))
    cases.append(_case("sml_host_graph_propagate",
                       [("src", z["w_item"]), ("elem_bytes", 4), ("d", D), ("n_src", N_ITEM), ("set_off", z["u_off"]), ("set_items", z["u_items"]),
                        ("rows", z["users"]), ("n", N), ("a", z["a"]), ("b", z["b"]), ("out", _out_f32(N, D))],
                       [("elem_bytes_8", {"elem_bytes": 8}), ("d_48", {"d": 48}), ("n_src_0", {"n_src": 0}), ("n_2^31", {"n": 1 << 31}),
                        ("set_off_alone", {"set_items": None}), ("set_items_alone", {"set_off": None}), ("n_0", {"n": 0}), ("src_null", {"src": None}),
                        ("out_null", {"out": None}), ("no_set", {"set_off": None, "set_items": None}), ("no_a_b", {"a": None, "b": None}),
                        ("out_on_src", {"out": At("src")}), ("out_on_set_off", {"out": At("set_off")}), ("out_on_set_items", {"out": At("set_items")}),
                        ("out_on_rows", {"out": At("rows")}), ("out_on_a", {"out": At("a")}), ("out_on_b", {"out": At("b", 156)}),
                        ("out_on_a_2nd_entry", {"out": At("a", 4)}), ("no_rows_out_on_a_2nd_entry", {"rows": None, "out": At("a", 4)}),
                        ("no_rows_out_on_set_off_2nd_entry", {"rows": None, "out": At("set_off", 8)}),
                        ("out_behind_b", {"out": At("b", 4 * N_ITEM)})]))
    rr_out = [("items", _i32(N, K)), ("pos", _i32(N, K)), ("value", _out_f32(N, K)), ("n_sel", _i32(N)), ("sim_sum", _out_f32(N))]
    rr_names = [n for n, _ in rr_out]
    cases.append(_case("sml_host_rerank_mmr",
                       [("w_item", z["w_item"]), ("elem_bytes", 4), ("d", D), ("n_item", N_ITEM), ("pool_items", z["pool_items"]), ("pool_rel", z["pool_rel"]),
                        ("n", N), ("pool_cols", 8), ("pool_stride", 8), ("nrm", z["nrm"]), ("lam", 0.5), ("normalize", 0), ("k", K)] + rr_out,
                       [("elem_bytes_3", {"elem_bytes": 3}), ("d_128_fp32", {"d": 128}), ("n_item_0", {"n_item": 0}), ("n_negative", {"n": -1}),
                        ("pool_cols_0", {"pool_cols": 0}), ("pool_cols_129", {"pool_cols": 129, "pool_stride": 129}), ("pool_stride_short", {"pool_stride": 7}),
                        ("k_0", {"k": 0}), ("k_129", {"k": 129}), ("lam_above_1", {"lam": 1.5}), ("lam_nan", {"lam": float("nan")}), ("normalize_2", {"normalize": 2}),
                        ("n_0", {"n": 0}), ("w_item_null", {"w_item": None}), ("pool_rel_null", {"pool_rel": None}), ("sim_sum_null", {"sim_sum": None}),
                        ("no_nrm", {"nrm": None}), ("w_item_misaligned", {"w_item": At("w_item", 4)}),
                        ("items_on_w_item", {"items": At("w_item")}), ("pos_on_pool_items", {"pos": At("pool_items", 64)}),
                        ("value_on_pool_rel", {"value": At("pool_rel")}), ("n_sel_on_nrm", {"n_sel": At("nrm", 156)}), ("sim_sum_on_w_item", {"sim_sum": At("w_item", 5116)}),
                        ("sim_sum_behind_nrm", {"sim_sum": At("nrm", 4 * N_ITEM)})]
                       + [("%s_on_%s" % (rr_names[b], rr_names[a]), {rr_names[b]: At(rr_names[a])}) for a in range(5) for b in range(a + 1, 5)]))
    cases.append(_case("sml_host_sample_negatives_ex",
                       [("users", z["users"]), ("n", N), ("item_all", z["item_all"]), ("pop", N_ITEM), ("user_ptr", z["u_off"]), ("n_users", N_USER),
                        ("user_items", z["u_items64"]), ("cdf", None), ("pool", 2), ("w_user", z["w_user"]), ("w_item", z["w_item"]), ("d", D), ("seed", 7),
                        ("negs", np.zeros(N, np.int64)), ("score", _out_f32(N)), ("failed", _i32(1))],
                       [("n_negative", {"n": -1}), ("pop_0", {"pop": 0}), ("n_users_negative", {"n_users": -1}), ("pool_0", {"pool": 0}), ("pool_65", {"pool": 65}),
                        ("users_null", {"users": None}), ("failed_null", {"failed": None}), ("negs_null", {"negs": None}), ("w_user_null", {"w_user": None}),
                        ("pool_1_no_tables", {"pool": 1, "w_user": None, "w_item": None}), ("d_128", {"d": 128}), ("w_item_misaligned", {"w_item": At("w_item", 8)})]))
    ns = [("rows", z["ns_rows"]), ("n", N), ("n_cols", 2), ("g0", 12), ("n_cat", z["ns_ncat"]), ("order", z["ns_order"]), ("h_off", z["ns_hoff"]),
          ("n_user", N_USER), ("h_items", z["ns_hitems"]), ("h_since", z["ns_hsince"]), ("neg_num", 4), ("seed", 3), ("out", np.zeros((N, 6), np.int64)),
          ("failed", _i32(1))]
    cases.append(_case("sml_host_neg_sets", ns,
                       [("n_negative", {"n": -1}), ("n_cols_1", {"n_cols": 1}), ("g0_negative", {"g0": -1}), ("g0_plus_n_2^31", {"g0": (1 << 31) - 2}),
                        ("n_user_0", {"n_user": 0}), ("neg_num_0", {"neg_num": 0}), ("neg_num_4097", {"neg_num": 4097}), ("failed_null", {"failed": None}),
                        ("h_off_null", {"h_off": None}), ("rows_null", {"rows": None}), ("out_null", {"out": None}), ("n_0_no_rows", {"n": 0, "rows": None, "out": None}),
                        ("out_on_rows", {"out": At("rows", 40)}), ("out_on_n_cat", {"out": At("n_cat")}), ("out_on_h_off", {"out": At("h_off", 48)}),
                        ("out_on_order", {"out": At("order")}), ("out_on_order_2nd_entry", {"out": At("order", 4)}), ("out_on_h_items", {"out": At("h_items")}),
                        ("out_on_h_since", {"out": At("h_since")}), ("out_on_failed", {"out": At("failed")}), ("out_behind_rows", {"out": At("rows", 8 * N * 2)})]))
    cases.append(_case("sml_host_resolve_negatives",
                       [("users", z["users"]), ("n", N), ("cand", z["cand"]), ("m", 8), ("pairs", z["pairs"]), ("n_pairs", len(z["pairs"])), ("stride", 1000),
                        ("negs", np.zeros(N, np.int64)), ("consumed", np.zeros(1, np.int64)), ("resolved", np.zeros(1, np.int64))],
                       [("users_null", {"users": None}), ("resolved_null", {"resolved": None}), ("n_negative", {"n": -1}), ("m_negative", {"m": -1}),
                        ("n_pairs_negative", {"n_pairs": -1}), ("stride_0", {"stride": 0})]))
    cases.append(_case("sml_host_resolve_negatives_csr",
                       [("users", z["users"]), ("n", N), ("cand", z["cand"]), ("m", 8), ("user_ptr", z["u_off"]), ("n_users", N_USER), ("user_items", z["u_items64"]),
                        ("negs", np.zeros(N, np.int64)), ("consumed", np.zeros(1, np.int64)), ("resolved", np.zeros(1, np.int64))],
                       [("cand_null", {"cand": None}), ("user_items_null", {"user_items": None}), ("n_negative", {"n": -1}), ("m_negative", {"m": -1}),
                        ("n_users_negative", {"n_users": -1})]))
    cases.append(_case("sml_host_gather_pairs",
                       [("ui", z["ui"]), ("n_rows", len(z["ui"])), ("order", z["order3"]), ("n", 3), ("out3", np.zeros((3, 3), np.int64))],
                       [("ui_null", {"ui": None}), ("n_negative", {"n": -1}), ("n_rows_negative", {"n_rows": -1}), ("index_outside", {"n_rows": 9}),
                        ("index_negative", {"order": np.array([4, -1, 9], np.int64)})]))
    cases.append(_case("sml_host_gather_column",
                       [("mat", z["mat"]), ("n_rows", 30), ("row_stride_bytes", 24), ("elem_bytes", 8), ("col", 1), ("order", z["order3"]), ("n", 3),
                        ("out3", np.zeros((3, 3), np.int64)), ("out_col", 2)],
                       [("mat_null", {"mat": None}), ("elem_bytes_2", {"elem_bytes": 2}), ("out_col_3", {"out_col": 3}), ("col_negative", {"col": -1}),
                        ("n_negative", {"n": -1}), ("index_outside", {"n_rows": 9})]))
    return cases


def gpu_cases():
    """Checks that only a call with a context reaches.  See the module docstring for what makes each of them harmless."""
    z = Z
    cases = []
    scratch = np.zeros(8, np.uint8)          # (Mem.put pads it to SCRATCH: see run)
    seen = [("seen_off", z["u_off"]), ("seen_items", z["u_items"])]
    rows = np.array([[0, 3, 5], [2, 1, 8], [4, 9, 30]], np.int64)
    pos_off, pos_items = np.array([0, 2, 3, 5], np.int64), np.array([1, 2, 11, 5, 6], np.int32)
    for suffix in ("", "_f16", "_filtered", "_adjusted"):
        f16, filt, adj = suffix == "_f16", suffix in ("_filtered", "_adjusted"), suffix == "_adjusted"
        tabs = [("ctx", Ctx()), ("w_user", z["w_user_h" if f16 else "w_user"]), ("w_item", z["w_item_h" if f16 else "w_item"])]
        tabs += [("elem_bytes", 4)] if adj else []
        tabs += [("n_item", N_ITEM)]
        extra = ([("allow", z["allow"])] if filt else []) + ([("adj", z["adj"])] if adj else [])
        muts = [("n_item_0", {"n_item": 0})]
        muts += [("ctx_d_128_fp32", {"ctx": Ctx(128)})] if not f16 else []
        muts += [("elem_bytes_3", {"elem_bytes": 3}), ("adj_misaligned", {"adj": At("adj", 4)})] if adj else []
        cases.append(_case("sml_full_rank" + suffix,
                           tabs + [("rows", rows), ("n", N), ("n_cols", 3)] + seen + extra + [("rank", _i32(N, 2)), ("stream", None)],
                           muts + [("n_cols_1", {"n_cols": 1})]))
        cases.append(_case("sml_topk_items" + suffix,
                           tabs + [("users", z["users"]), ("n", N), ("k", K)] + seen + extra
                           + [("scratch", scratch), ("items", _i32(N, K)), ("scores", _out_f32(N, K)), ("stream", None)], muts))
        cases.append(_case("sml_user_rank" + suffix,
                           tabs + [("users", z["users"]), ("n", N), ("pos_off", pos_off), ("pos_items", pos_items), ("n_pos", 5)] + seen + extra
                           + [("scratch", scratch), ("above", _i32(5)), ("pos", _i32(5)), ("stream", None)], muts))
    head = [("ctx", Ctx()), ("w_user", z["w_user"]), ("w_item", z["w_item"]), ("elem_bytes", 4), ("n_item", N_ITEM), ("users", z["users"]), ("n", N)]
    tail = seen + [("allow", z["allow"]), ("adj", z["adj"])]
    outs = [("items", _i32(N, K)), ("scores", _out_f32(N, K)), ("n_elig", _i32(N)), ("stream", None)]
    tabs_mis = [("adj_misaligned", {"adj": At("adj", 4)}), ("w_user_misaligned", {"w_user": At("w_user", 4)}), ("w_item_misaligned", {"w_item": At("w_item", 8)})]
    cand = np.array([[1, 2, 5, 6, 9, 11], [0, 3, 4, 7, 8, 10], [12, 13, 14, 15, 16, 17]], np.int32)
    cases.append(_case("sml_topk_candidates",
                       head + [("cand", cand), ("cand_elem_bytes", 4), ("cand_off", None), ("cand_stride", 6), ("cand_first", 0), ("cand_cols", 6), ("k", K)]
                       + tail + [("max_workgroups", 0)] + outs,
                       tabs_mis + [("elem_bytes_3", {"elem_bytes": 3}), ("cand_elem_bytes_2", {"cand_elem_bytes": 2}), ("cand_cols_negative", {"cand_cols": -1}),
                                   ("n_item_0", {"n_item": 0}), ("ctx_d_128_fp32", {"ctx": Ctx(128)}), ("items_on_users", {"items": At("users")}),
                                   ("scores_on_cand", {"scores": At("cand", 68)}), ("n_elig_on_w_user", {"n_elig": At("w_user", 124)}),
                                   ("items_on_adj", {"items": At("adj")}), ("scores_on_items", {"scores": At("items")}),
                                   ("n_elig_on_scores", {"n_elig": At("scores", 44)}), ("n_elig_on_items", {"n_elig": At("items")})]))
    cases.append(_case("sml_ivf_search",
                       head + [("list_off", z["list_off"]), ("list_items", z["list_items"]), ("n_list", N_LIST), ("probes", z["probes"]), ("nprobe", NPROBE),
                               ("k", K)] + tail + [("max_workgroups", 0)] + outs, tabs_mis + [("max_workgroups_negative", {"max_workgroups": -1})]))
    cases.append(_case("sml_topk_deep", head + [("k", K)] + tail + [("slices", 0), ("scratch", scratch)] + outs,
                       tabs_mis + [("scratch_misaligned", {"scratch": At("scratch", 16)}), ("slices_negative", {"slices": -1})]))
    cases.append(_case("sml_gram",
                       [("ctx", Ctx()), ("w", z["w_item"]), ("elem_bytes", 4), ("n_rows", N_ITEM), ("scratch", scratch), ("gram", np.zeros((D, D))), ("stream", None)],
                       [("scratch_misaligned", {"scratch": At("scratch", 8)}), ("gram_misaligned", {"gram": At("gram", 8)}),
                        ("gram_on_scratch", {"gram": At("scratch", 256)})]))
    cases.append(_case("sml_als_solve",
                       [("ctx", Ctx()), ("w_other", z["w_item"]), ("elem_bytes", 4), ("n_other", N_ITEM), ("gram", z["gram"]), ("alpha0", 0.5), ("reg", 0.1),
                        ("set_off", z["u_off"]), ("set_items", z["u_items"]), ("rows", z["users"]), ("n", N), ("w_out", _out_f32(N_USER, D)), ("n_out", N_USER),
                        ("max_workgroups", 0), ("status", _i32(N)), ("stream", None)],
                       [("gram_misaligned", {"gram": At("gram", 8)}), ("max_workgroups_negative", {"max_workgroups": -1})]))
    cases.append(_case("sml_cooc_topk",
                       [("ctx", Ctx()), ("by_item_off", z["i_off"]), ("by_item_users", z["i_users"]), ("by_user_off", z["u_off"]), ("by_user_items", z["u_items"]),
                        ("n_user", N_USER), ("n_item", N_ITEM), ("rows", z["users"]), ("n", N), ("norm_a", z["norm"]), ("norm_b", z["norm"].copy()), ("shrink", 1.0),
                        ("min_co", 1), ("allow", z["allow"]), ("k", K), ("max_workgroups", 0), ("path", 0), ("scratch", scratch), ("items", _i32(N, K)),
                        ("sims", _out_f32(N, K)), ("n_elig", _i32(N)), ("stream", None)],
                       [("scratch_misaligned", {"scratch": At("scratch", 16)}), ("items_on_scratch", {"items": At("scratch", 256)}), ("max_workgroups_negative", {"max_workgroups": -1})]))
    cases.append(_case("sml_knn_topk",
                       [("ctx", Ctx()), ("nbr_items", z["nbr_items"]), ("nbr_sims", z["nbr_sims"]), ("n_rows_nbr", N_ITEM), ("k_nbr", 4), ("n_item", N_ITEM),
                        ("hist_off", z["u_off"]), ("hist_items", z["u_items"]), ("users", z["users"]), ("n", N), ("frac_bits", 16), ("seen_off", z["u_off"].copy()),
                        ("seen_items", z["u_items"].copy()), ("allow", z["allow"]), ("k", K), ("max_workgroups", 0), ("path", 0), ("scratch", scratch),
                        ("items", _i32(N, K)), ("scores", _out_f32(N, K)), ("n_elig", _i32(N)), ("stream", None)],
                       [("scratch_misaligned", {"scratch": At("scratch", 16)}), ("n_elig_on_scratch", {"n_elig": At("scratch", 512)}), ("max_workgroups_negative", {"max_workgroups": -1})]))
    cases.append(_case("sml_graph_propagate",
                       [("ctx", Ctx()), ("src", z["w_item"]), ("elem_bytes", 4), ("n_src", N_ITEM), ("set_off", z["u_off"]), ("set_items", z["u_items"]),
                        ("rows", z["users"]), ("n", N), ("a", z["a"]), ("b", z["b"]), ("max_workgroups", 0), ("path", 0), ("scratch", scratch),
                        ("out", _out_f32(N, D)), ("stream", None)],
                       [("scratch_misaligned", {"scratch": At("scratch", 16)}), ("src_misaligned", {"src": At("src", 4)}), ("out_misaligned", {"out": At("out", 8)}),
                        ("out_on_scratch", {"out": At("scratch", 256)}), ("max_workgroups_negative", {"max_workgroups": -1})]))
    irows = np.array([[u, i, 0] for u in range(N_USER) for i in ((7 * u) % N_ITEM, (7 * u + 3) % N_ITEM)], np.int64)
    cases.append(_case("sml_iset_build",
                       [("ctx", Ctx()), ("rows", irows), ("m", len(irows)), ("n_cols", 3), ("n_user", N_USER), ("n_item", N_ITEM), ("scratch", scratch),
                        ("off", np.zeros(N_USER + 1, np.int64)), ("items", _i32(len(irows))), ("stream", None)],
                       [("n_cols_1", {"n_cols": 1}), ("scratch_misaligned", {"scratch": At("scratch", 8)})]))
    b_off, b_items = np.arange(N_USER + 1, dtype=np.int64), np.array([39, 38, 37, 36, 35, 34], np.int32)
    nnz_a = len(z["u_items"])
    cases.append(_case("sml_iset_union",
                       [("ctx", Ctx()), ("n_user", N_USER), ("a_off", z["u_off"]), ("a_items", z["u_items"]), ("nnz_a", nnz_a), ("b_off", b_off),
                        ("b_items", b_items), ("nnz_b", 6), ("scratch", scratch), ("out_off", np.zeros(N_USER + 1, np.int64)), ("out_items", _i32(nnz_a + 6)),
                        ("stream", None)],
                       [("n_user_0", {"n_user": 0}), ("scratch_misaligned", {"scratch": At("scratch", 8)}), ("out_off_on_a_off", {"out_off": At("a_off")}),
                        ("out_off_on_b_off", {"out_off": At("b_off", 48)}), ("out_items_on_a_items", {"out_items": At("a_items")}),
                        ("out_items_on_b_items", {"out_items": At("b_items", 20)}), ("out_off_on_a_items", {"out_off": At("a_items")}),
                        ("out_off_on_b_items", {"out_off": At("b_items")}), ("out_items_on_a_off", {"out_items": At("a_off")}),
                        ("out_items_on_b_off", {"out_items": At("b_off")})]))
    cases.append(_case("sml_item_adjust_fill",
                       [("ctx", Ctx()), ("scale", np.ones(N_ITEM, np.float32)), ("offset", np.zeros(N_ITEM, np.float32)), ("n_item", N_ITEM),
                        ("adj", np.zeros(128, np.float32)), ("stream", None)],
                       [("n_item_0", {"n_item": 0}), ("adj_misaligned", {"adj": At("adj", 4)})]))
    cases.append(_case("sml_item_adjust_cosine",
                       [("ctx", Ctx()), ("w_item", z["w_item"]), ("elem_bytes", 4), ("n_item", N_ITEM), ("adj", np.zeros(128, np.float32)), ("stream", None)],
                       [("elem_bytes_3", {"elem_bytes": 3}), ("ctx_d_128_fp32", {"ctx": Ctx(128)}), ("n_item_0", {"n_item": 0}),
                        ("adj_misaligned", {"adj": At("adj", 8)})]))
    cases.append(_case("sml_item_filter_from_ids",
                       [("ctx", Ctx()), ("ids", np.array([1, 5, 39], np.int32)), ("n_ids", 3), ("n_item", N_ITEM), ("invert", 0), ("words", np.zeros(2, np.uint32)),
                        ("stream", None)],
                       [("invert_2", {"invert": 2}), ("n_item_0", {"n_item": 0})]))
    cases.append(_case("sml_user_metrics",
                       [("ctx", Ctx()), ("pos", np.array([0, 3, 1, 7, 2], np.int32)), ("pos_off", pos_off), ("n", N), ("ks", Host(np.array([1, 5], np.int32))),
                        ("n_k", 2), ("hits", _i32(N, 2)), ("dcg", _out_f32(N, 2)), ("ap", _out_f32(N, 2)), ("first", _i32(N)), ("stream", None)],
                       [("n_k_0", {"n_k": 0}), ("ks_holds_0", {"ks": Host(np.array([1, 0], np.int32))})]))
    return cases


def run(lib, cases, device=None, ctx_of=None):
    """{"<fn>:<label>": [return code, sml_last_error() text]} of the valid call ("valid") and every mutation, in order."""
    from sml_amd import _lib
    out = {}
    for c in cases:
        mem = Mem(device)
        fn = getattr(lib, c["fn"])
        argtypes = _lib.SIGNATURES[c["fn"]][1]
        assert len(argtypes) == len(c["args"]), c["fn"]
        placed = {}

        def place(name, v):
            if isinstance(v, np.ndarray):
                if name == "scratch":
                    v = np.zeros(SCRATCH, np.uint8)
                return mem.put(v)
            if isinstance(v, Host):
                return mem.put(v.arr, host=True)
            return v
        for name, v in c["args"]:
            placed[name] = place(name, v)

        def call(over):
            vals = dict(placed)
            for name, v in over.items():
                assert name in vals, (c["fn"], name)
                vals[name] = place(name, v)
            final = []
            for (name, _), t in zip(c["args"], argtypes):
                v = vals[name]
                if isinstance(v, At):
                    v = placed[v.name] + v.off
                elif isinstance(v, Ctx):
                    v = ctx_of(v.d)
                if isinstance(v, int) and isinstance(t, type) and issubclass(t, ctypes._Pointer):
                    v = ctypes.cast(v, t)
                final.append(v)
            rc = fn(*final)
            msg = lib.sml_last_error() if rc != 0 else b""
            return [int(rc), msg.decode()]
        out[c["fn"] + ":valid"] = call({})
        for label, over in c["muts"]:
            key = c["fn"] + ":" + label
            assert key not in out, key
            out[key] = call(over)
        if device is not None:
            import torch
            torch.cuda.synchronize()
    return out


def scratch_needs(lib, ctx):
    """The largest scratch any valid GPU call above asks for, by the library's own answers."""
    nnz_a = len(Z["u_items"])
    return max(lib.sml_topk_scratch_bytes(ctx, N, K, N_ITEM), lib.sml_user_rank_scratch_bytes(ctx, N, 5, N_ITEM),
               lib.sml_topk_deep_scratch_bytes(ctx, N, K, N_ITEM, 0), lib.sml_gram_scratch_bytes(ctx, N_ITEM),
               lib.sml_knn_scratch_bytes(ctx, N_ITEM, 0, 0), lib.sml_knn_scratch_bytes(ctx, N_ITEM, 0, 1),
               lib.sml_graph_scratch_bytes(ctx, N, nnz_a, 0), lib.sml_iset_build_scratch_bytes(ctx, 2 * N_USER, N_USER, N_ITEM),
               lib.sml_iset_union_scratch_bytes(ctx, nnz_a, 6, N_USER))


class Contexts:
    """ctx_of(d) for the GPU cases: one context per embedding width on device 0, destroyed on exit; checks the scratch block."""
    def __init__(self, lib):
        self.lib, self.made = lib, {}

    def __enter__(self):
        import ctypes
        def ctx_of(d):
            if d not in self.made:
                h = ctypes.c_void_p()
                assert self.lib.sml_ctx_create(ctypes.byref(h), 0, d, 256) == 0, self.lib.sml_last_error()
                self.made[d] = h
            return self.made[d]
        assert 0 < scratch_needs(self.lib, ctx_of(D)) <= SCRATCH
        return ctx_of

    def __exit__(self, *exc):
        for h in self.made.values():
            self.lib.sml_ctx_destroy(h)
        self.made = {}


def recorded(section):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_capi_refusals.json")) as f:
        return json.load(f)[section]


def assert_same(got, want):
    assert sorted(got) == sorted(want), "the cases and the recording name different calls"
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, "\n".join("%s: got %r, recorded %r" % (k, g, w) for k, (g, w) in sorted(diff.items()))
