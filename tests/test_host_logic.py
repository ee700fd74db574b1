"""Host-side logic on CPU: batch supply (G8), parameter initialisation (G9), the CLI,
the C-ABI library's exported symbols, and the driver's control flow / printed lines
against the reference's end-to-end log (G7) with the CPU oracle injected as the
engine (the product itself has no CPU path; see sml_amd/driver.py:_make_engine)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, golden, quiet
from oracle import sml_oracle as O


# ----------------------------------------------------------------------------- G8
def test_g8_presample_batches_match_dataloader_order():
    from sml_amd import datasets as D
    z = golden("g8_batches.npz")
    table = z["table"]
    torch.manual_seed(501)
    np.random.seed(502)
    ds = D.trainDataset_withPreSample(table)
    got = [ds.epoch_triples(D.loader_order(len(ds))) for _ in range(8)]
    np.testing.assert_array_equal(np.concatenate(got, 0), z["presample_seq"])


def test_g8_rejection_sampling_matches_per_item_draws():
    from sml_amd import datasets as D
    z = golden("g8_batches.npz")
    torch.manual_seed(503)
    np.random.seed(504)
    with quiet():
        ds = D.offlineDataset_withsample(z["pairs"])
    got = [ds.epoch_triples(D.loader_order(len(ds))) for _ in range(3)]
    np.testing.assert_array_equal(np.concatenate(got, 0), z["withsample_seq"])
    # and the numpy generator is left exactly where per-item draws leave it
    np.random.seed(7)
    with quiet():
        a = D.offlineDataset_withsample(z["pairs"])
    order = np.arange(len(a))
    vec = a.epoch_triples(order)
    after_vec = np.random.randint(0, 1 << 30)
    np.random.seed(7)
    with quiet():
        b = D.offlineDataset_withsample(z["pairs"])
    seq = np.array([b[i] for i in order], dtype=np.int64)
    after_seq = np.random.randint(0, 1 << 30)
    np.testing.assert_array_equal(vec, seq)
    assert after_vec == after_seq


def test_epoch_speculation_is_exact_or_discarded():
    """datasets.EpochSpeculation (the transfer stage's next pass drawn ahead on a helper thread): adopted, it yields the very
    triples and leaves both generators (and the module's draw counter) exactly where the in-place sequence [MF constructor shuffle, 2 torch draws per MF epoch,
    loader_order, epoch_triples] leaves them; with a wrong prediction (another numpy draw in between, another order, another
    dataset) it yields None and touches neither generator.  Data: G8's pairs (data/dataset.py:41-71)."""
    from sml_amd import datasets as D
    z = golden("g8_batches.npz")
    with quiet():
        ds = D.offlineDataset_withsample(z["pairs"])
        other = D.offlineDataset_withsample(z["pairs"])
    cols, mf_epochs = 1000, 2

    def in_place():
        np.random.shuffle(np.arange(1, cols + 1))               # trainDataset_withPreSample.__init__
        for _ in range(mf_epochs):
            D.loader_order(123)                                  # the MF epochs' DataLoader draws
        order = D.loader_order(len(ds))
        return order, ds.epoch_triples(order)

    def states():
        return np.random.get_state(), torch.get_rng_state(), D.torch_draws()

    def same(a, b):
        return D._same_rng_state(a[0], b[0]) and torch.equal(a[1], b[1])

    torch.manual_seed(11); np.random.seed(12)
    order_ref, tri_ref = in_place()
    end_ref = states()
    # the speculated path: started BEFORE the intermediate draws, adopted after them
    torch.manual_seed(11); np.random.seed(12)
    spec = D.EpochSpeculation(ds, torch_draws_before=2 * mf_epochs, np_shuffles_before=(cols,))
    start = states()
    torch.manual_seed(11); np.random.seed(12)
    assert same(start, states()), "starting a speculation moved a generator"
    np.random.shuffle(np.arange(1, cols + 1))
    for _ in range(mf_epochs):
        D.loader_order(123)
    order = D.loader_order(len(ds))
    np.testing.assert_array_equal(order, order_ref)
    got = spec.adopt(ds, order)
    assert got is not None
    np.testing.assert_array_equal(got, tri_ref)
    assert same(states(), end_ref)
    # wrong predictions: discarded, generators untouched, the in-place path still gives the reference result
    for case in ("extra numpy draw", "other order", "other dataset", "no shuffle predicted"):
        torch.manual_seed(11); np.random.seed(12)
        spec = D.EpochSpeculation(ds, 2 * mf_epochs, (cols,) if case != "no shuffle predicted" else ())
        np.random.shuffle(np.arange(1, cols + 1))
        if case == "extra numpy draw":
            np.random.randint(0, 10)
        for _ in range(mf_epochs):
            D.loader_order(123)
        order = D.loader_order(len(ds))
        before = states()
        if case == "other order":
            assert spec.adopt(ds, order[::-1].copy()) is None
        elif case == "other dataset":
            assert spec.adopt(other, order) is None
        else:
            assert spec.adopt(ds, order) is None
        assert same(states(), before), case
    # the next epoch of the same call: no draws predicted in between
    torch.manual_seed(21); np.random.seed(22)
    o1 = D.loader_order(len(ds)); t1 = ds.epoch_triples(o1)
    o2 = D.loader_order(len(ds)); t2 = ds.epoch_triples(o2)
    end = states()
    torch.manual_seed(21); np.random.seed(22)
    o1b = D.loader_order(len(ds)); t1b = ds.epoch_triples(o1b)
    spec = D.EpochSpeculation(ds)
    o2b = D.loader_order(len(ds))
    t2b = spec.adopt(ds, o2b)
    np.testing.assert_array_equal(t1b, t1)
    assert t2b is not None
    np.testing.assert_array_equal(t2b, t2)
    assert same(states(), end)


def test_presample_getitem_equals_epoch_triples():
    from sml_amd import datasets as D
    z = golden("g8_batches.npz")
    np.random.seed(1)
    a = D.trainDataset_withPreSample(z["table"])
    np.random.seed(1)
    b = D.trainDataset_withPreSample(z["table"])
    for _ in range(7):   # crosses the neg_flag reshuffle
        order = np.random.RandomState(0).permutation(len(a))
        st = np.random.get_state()
        va = a.epoch_triples(order)
        np.random.set_state(st)
        vb = np.array([b[i] for i in order], dtype=np.int64)
        np.testing.assert_array_equal(va, vb)


# ----------------------------------------------------------------------------- G9
def test_g9_parameter_init_order():
    from model.MF import MFbasemode
    from model.conv_transfer import ConvTransfer_com
    z = golden("g9_init.npz")
    torch.manual_seed(2000)
    mf = MFbasemode(37, 23, 32)
    with quiet():
        net = ConvTransfer_com(32, 32)
    assert list(mf.state_dict().keys()) == list(z["mf_keys"])
    assert list(net.state_dict().keys()) == list(z["theta_keys"])
    for k, v in mf.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), z["mf." + k])
    for k, v in net.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), z["theta." + k])


def test_reference_checkpoint_unpickles_as_our_class():
    import model.MF
    mf = torch.load(os.path.join(GOLDEN, "ref_BCE_init_tiny.pkl"), map_location="cpu", weights_only=False)
    assert type(mf) is model.MF.MFbasemode
    z = golden("g7_end_to_end.npz")
    np.testing.assert_array_equal(mf.user_laten.weight.detach().numpy(), z["mf.user_laten.weight"])
    assert (mf.user_num, mf.item_num, mf.hidden_dim) == (300, 120, 32)


# ----------------------------------------------------------------------------- CLI
def test_cli_defaults_and_quirks():
    import main_news
    import main_yelp
    y = main_yelp.get_parse().parse_args([])
    n = main_news.get_parse().parse_args([])
    assert (y.data_name, y.multi_num, y.MF_epochs, y.TR_epochs, y.MF_batch_size, y.TR_batch_size) == ("yelp", 10, 1, 1, 1024, 256)
    assert (n.data_name, n.multi_num, n.MF_epochs, n.TR_epochs) == ("news", 7, 2, 2)
    assert (y.MF_lr, y.l2, y.TR_lr, y.TR_l2, y.laten, y.seed, y.topK) == (0.01, 1e-6, 0.001, 1e-4, 64, 2000, 20)
    # type=bool is truthy for any non-empty string, as in the reference
    assert main_yelp.get_parse().parse_args(["--TR_stop_", "False"]).TR_stop_ is True
    assert main_yelp.get_parse().parse_args(["--clip_grad", "0"]).clip_grad == "0"


# ----------------------------------------------------------------------------- C ABI
def test_capi_exports_every_declared_symbol():
    from sml_amd import _lib
    hdr = open(os.path.join(REPO, "include", "sml_hip.h")).read()
    declared = set(re.findall(r"\b(sml_[a-z0-9_]+)\s*\(", hdr)) - {"sml_grad_hook"}
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.sml_version() >= 1
    # layout facts the host relies on; no GPU needed for these
    assert lib.sml_theta_net_size(32) >= 98943 and lib.sml_theta_net_size(48) == -1
    offs = [lib.sml_theta_offset(32, w) for w in range(8)]
    assert offs == sorted(offs) and all(o % 4 == 0 for o in offs)


def test_product_has_no_cpu_path():
    """The product fails loudly without a GPU / library instead of falling back."""
    from sml_amd import engine
    from sml_amd.mf import MFbasemode
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        engine.HipEngine("cuda:0", 32)
    mf = MFbasemode(4, 4, 32)
    with pytest.raises(RuntimeError):
        mf.test(torch.zeros(2, 5, dtype=torch.long))
    for mod in ("sml_amd/engine.py", "sml_amd/driver.py", "sml_amd/mf.py", "sml_amd/conv_transfer.py",
                "sml_amd/evaluation.py", "sml_amd/datasets.py", "sml_amd/cli.py", "sml_amd/_lib.py"):
        src = open(os.path.join(REPO, mod)).read()
        assert "oracle" not in src.replace("no CPU", ""), mod


# ----------------------------------------------------------------------------- G7 on CPU
class _CpuEngine(O.OracleEngine):
    """Test double with HipEngine's surface."""

    def __init__(self, device, d, max_batch):
        O.OracleEngine.__init__(self, d)

    def mf_stage_epoch(self, mfbase, transfer, last_user, last_item, triples, *a, **k):
        return O.OracleEngine.mf_stage_epoch(self, mfbase, transfer, last_user, last_item,
                                             torch.as_tensor(triples), *a, **k)

    def tr_stage_epoch(self, transfer, lu, li, hu, hi, triples, *a, **k):
        return O.OracleEngine.tr_stage_epoch(self, transfer, lu, li, hu, hi, torch.as_tensor(triples), *a, **k)


def _cpu_mf_test(self, inputs_data, topK=20):
    ranks = O.eval_ranks(self.user_laten.weight.data, self.item_laten.weight.data, inputs_data)
    hits, ndcg = O.eval_metrics(ranks, topK)
    return hits, (torch.tensor(ndcg) if hits > 0 else 0), (ranks < topK).nonzero()[:, 0]


_NUM = re.compile(r"-?\d+\.\d+(?:e-?\d+)?|-?\d+")


def compare_logs(got, want, exact_lines):
    """Line-by-line: same text everywhere (timing lines and tmp paths aside).  Numbers: the
    first `exact_lines` lines agree to the printed digit.  After that a free-running fp32
    trajectory drifts -- Adam divides rounding noise by sqrt(v), and mid-training recall on
    160 rows moves in steps of 1/160; the fp32 CPU oracle itself drifts from the fp32 CPU
    reference this way -- so later numbers are compared as a distribution.
    Returns the absolute differences of all later recall/ndcg/loss numbers."""
    def lines(log):
        log = re.sub(r"\[[^\]]*\]", lambda m: "[" + " ".join(m.group(0)[1:-1].split()) + "]", log)   # un-wrap numpy array prints
        return [" ".join(l.split()) for l in log.splitlines() if "time cost" not in l and not l.startswith("Namespace(")]
    g, w = lines(got), lines(want)
    assert len(g) == len(w), (len(g), len(w))
    diffs = []
    for ln, (a, b) in enumerate(zip(g, w)):
        if a == b:
            continue
        if "set_tt is:" in a or "settt is:" in a:      # path prefix differs (tmp dir)
            assert a.split("/")[-2:] == b.split("/")[-2:]
            continue
        assert _NUM.sub("#", a) == _NUM.sub("#", b), (a, b)
        for x, y in zip(_NUM.findall(a), _NUM.findall(b)):
            x, y = float(x), float(y)
            if ln < exact_lines:
                assert abs(x - y) <= 1.01e-4 * max(1.0, abs(y)), (ln, a, b)
            else:
                diffs.append(abs(x - y))
    return np.array(diffs if diffs else [0.0])


def check_g7(got, want, exact_lines):
    d = compare_logs(got, want, exact_lines)
    assert np.median(d) <= 2e-3, np.median(d)
    assert np.percentile(d, 90) <= 0.025, np.percentile(d, 90)
    fin = lambda log, key: float([l for l in log.splitlines() if l.startswith(key)][0].split(":")[1])
    for key in ("test average recall@20", "test average ndcg@20", "val average recall@20", "val average ndcg@20"):
        assert abs(fin(got, key) - fin(want, key)) <= 0.02, key


def run_g7(tmp_path, monkeypatch, device_patch=True, variant=""):
    from sml_amd import cli, driver, synth
    from sml_amd.mf import MFbasemode
    # "_conv": the same run with --transfer_type conv; "_news": main_news.py (63 periods, multi_num 7, 2 + 2 epochs)
    z = golden("g7_end_to_end%s.npz" % variant)
    which = "news" if variant == "_news" else "yelp"
    P, n_inter, U, I, neg, seed = [int(v) for v in z["dataset"]]
    root = str(tmp_path) + "/"
    synth.write_dataset(root, which, n_periods=P, n_inter=n_inter, n_user=U, n_item=I, neg=neg,
                        a_user=float(z["dataset_zipf"][0]), a_item=float(z["dataset_zipf"][1]), seed=seed)
    mf = MFbasemode(U, I, 32)
    mf.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("mf.")})
    ck = os.path.join(root, "BCE_init.pkl")
    torch.save(mf, ck)
    argv = ["--data_path", root, "--pre_model", ck] + [str(a) for a in z["argv"]]
    with quiet() as buf:
        cli.main(which, argv)
    return buf.getvalue(), str(z["log"])


@pytest.mark.parametrize("variant", ["", "_conv", "_news"])
def test_g7_driver_control_flow_on_cpu(tmp_path, monkeypatch, variant):
    from sml_amd import driver
    from sml_amd.mf import MFbasemode
    monkeypatch.setattr(driver, "_default_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(driver, "_make_engine", lambda dev, d, mb: _CpuEngine(dev, d, mb))
    monkeypatch.setattr(MFbasemode, "test", _cpu_mf_test)
    monkeypatch.delenv("CUDA_VISIBLE_DEVICES", raising=False)
    got, want = run_g7(tmp_path, monkeypatch, variant=variant)
    # identical data and RNG tape: the first three periods print identically
    check_g7(got, want, exact_lines=90)


# ----------------------------------------------------------------------------- G12 mid-size sequence
def g12_losses_from_log(log):
    """(kind, value) of every printed training loss / metric line, in order."""
    out = []
    for l in log.splitlines():
        if "time cost" in l:
            continue
        for m in re.finditer(r"(recall|reacll|ndcg|loss):\s*(-?\d+\.\d+)", l):
            out.append((m.group(1).replace("reacll", "recall"), float(m.group(2)), l))
    return out


def run_g12(tmp_path, teacher_forced, spy=None, name="g12_midsize"):
    """The product's period loop on G12's dataset, seeded and configured as tests/golden/make_golden.py: gen_g12 drove
    the reference (main_yelp.py's __main__ body with six periods).  teacher_forced: at the start of every stage
    the fixture holds a state for (2 and 3), tables, theta and both Adam states are set to the reference's.
    Returns (meta, log, per-batch losses [(stage, kind, value)...])."""
    from sml_amd import cli, datasets, driver, synth
    from sml_amd.mf import MFbasemode
    z = golden(name + ".npz")
    U, I, d, n_inter, neg, P, train_from, test_from, multi_num, seed, data_seed, ck_seed = [int(v) for v in z["config"]]
    root = str(tmp_path) + "/"
    synth.write_dataset(root, "yelp", n_periods=P, n_inter=n_inter, n_user=U, n_item=I, neg=neg,
                        a_user=float(z["zipf"][0]), a_item=float(z["zipf"][1]), seed=data_seed)
    torch.manual_seed(ck_seed)
    mf = MFbasemode(U, I, d)
    with torch.no_grad():
        mf.user_laten.weight.mul_(0.3)
        mf.item_laten.weight.mul_(0.3)
    ck = os.path.join(root, name + "_init.pkl")
    torch.save(mf, ck)
    args = cli.get_parse("yelp").parse_args(["--data_path", root, "--pre_model", ck, "--laten", str(d), "--multi_num",
                                            str(multi_num), "--numworkers", "0", "--seed", str(seed)])
    torch.set_num_threads(int(os.environ.get("SML_HOST_THREADS", "1")) if torch.cuda.is_available() else torch.get_num_threads())
    torch.manual_seed(args.seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(args.seed + 1)
    np.random.seed(args.seed + 2)
    batch_losses = []
    with quiet() as buf:
        sets = datasets.transfer_data(args, path=root, datasetname="yelp", file_path_list=[str(i) for i in range(P)],
                                      test_list=[str(j) for j in range(test_from, P)], validation_list=None,
                                      online_train_time=train_from, online_test_time=test_from)
        meta = driver.meta_train(args, sets, sets.user_number, sets.item_number, args.laten)
        for k in z.files:       # the transfer net's initial parameters are the reference's (seeded identically: G9)
            if k.startswith("theta0."):
                np.testing.assert_array_equal(meta.transfer.state_dict()[k[7:]].cpu().numpy(), z[k])
        eng = meta.engine
        stage_now = [0]
        for meth, kind in (("mf_stage_epoch", 0), ("tr_stage_epoch", 1)):
            def wrap(fn, kind=kind):
                def inner(*a, **k):
                    l = fn(*a, **k)
                    batch_losses.append((stage_now[0], kind, l))
                    return l
                return inner
            setattr(eng, meth, wrap(getattr(eng, meth)))
        real_stage = meta.train_one_stage3
        forced = []
        meta._forced_stages = forced          # (the tests assert that the forcing HAPPENED where the fixture holds a state)

        def stage(a, stage_id):
            stage_now[0] = stage_id
            path = os.path.join(GOLDEN, name + "_state_s%d.npz" % stage_id)
            if teacher_forced and os.path.exists(path):
                forced.append(stage_id)
                sn = np.load(path)
                dev = meta.MFbase.user_laten.weight.device
                meta.MFbase.user_laten.weight.data.copy_(torch.from_numpy(sn["W_user"]).to(dev))
                meta.MFbase.item_laten.weight.data.copy_(torch.from_numpy(sn["W_item"]).to(dev))
                meta.transfer.load_state_dict({k[6:]: torch.from_numpy(sn[k]) for k in sn.files if k.startswith("theta.")})
                names = [n for n, _ in meta.transfer.named_parameters()]
                eng.load_optimizer_state(
                    mfbase=meta.MFbase, transfer=meta.transfer,
                    mf_state=dict(m_user=sn["mf_m_user"], v_user=sn["mf_v_user"], m_item=sn["mf_m_item"],
                                  v_item=sn["mf_v_item"], step=int(sn["mf_step"])),
                    tr_state=dict(m={n: sn["tr_m." + n] for n in names}, v={n: sn["tr_v." + n] for n in names},
                                  step=int(sn["tr_step"])))
                meta._touch_tables()
            return real_stage(a, stage_id)
        meta.train_one_stage3 = stage
        meta.run(args)
    flat = []
    for st, kind, l in batch_losses:
        arr = l.detach().cpu().numpy() if isinstance(l, torch.Tensor) else np.asarray(l)
        flat += [(st, kind, float(v)) for v in arr]
    return meta, buf.getvalue(), flat, z


def g12_compare(log, want_log, flat, z, stages, loss_rtol, flips):
    """Inside `stages`: every per-batch loss within loss_rtol of the reference's backpropagated scalar, every
    printed recall within `flips` rank flips (n = 10,000 rows: one flip = 1e-4), ndcg within flips / n too.
    Returns (max loss rel err, max |recall diff|, max |ndcg diff|) over those stages."""
    tags, ref = z["batch_tag"], z["batch_loss"]
    assert len(flat) == len(ref) and all((a[0], a[1]) == (int(t[0]), int(t[1])) for a, t in zip(flat, tags))
    sel = np.isin(tags[:, 0], list(stages))
    got = np.array([a[2] for a in flat])
    rel = np.abs(got[sel] - ref[sel]) / np.abs(ref[sel])
    # printed metrics, stage by stage ("now time:" opens a stage's block of lines)
    def blocks(text):
        out, cur = [], None
        for l in text.splitlines():
            if l.startswith("now time:") and (cur is None or not cur[-1].startswith("now time:")) \
                    and (cur is None or not cur[-1].startswith("will be test")):
                if cur is not None and any("MF (inner)" in x for x in cur):
                    out.append(cur)
                    cur = []
                elif cur is None:
                    cur = []
            if cur is not None:
                cur.append(l)
        out.append(cur)
        return out
    gb, wb = blocks(log), blocks(want_log)
    assert len(gb) == len(wb) == int(tags[:, 0].max()) + 1, (len(gb), len(wb))
    dr, dn = [0.0], [0.0]
    for st in stages:
        g, w = g12_losses_from_log("\n".join(gb[st])), g12_losses_from_log("\n".join(wb[st]))
        assert [x[0] for x in g] == [x[0] for x in w]
        for (k, a, _), (_, b, _) in zip(g, w):
            if k == "recall":
                dr.append(abs(a - b))
            elif k == "ndcg":
                dn.append(abs(a - b))
    n = 10000.0
    assert rel.max() <= loss_rtol, "per-batch loss: max rel err %.3e" % rel.max()
    assert max(dr) <= flips / n + 1e-9, "recall: max diff %.4f" % max(dr)
    assert max(dn) <= flips / n + 0.5e-4 + 1e-9, "ndcg: max diff %.4f" % max(dn)      # (+ the print's own rounding)
    return rel.max(), max(dr), max(dn)


def test_g12_midsize_sequence_on_cpu_oracle(tmp_path, monkeypatch):
    """G12 through the product's driver with the oracle injected: control flow, RNG tape and the oracle's
    arithmetic against the reference at a size where Recall@20 resolves 1e-4.  Teacher-forced at stages 2 and 3
    (state set to the reference's at the stage start): per-batch losses to 2e-5 relative, Recall@20 within 2 rank
    flips; stage 0 (identical start by seed) to the same bar; the free-running gap is reported."""
    from sml_amd import driver
    from sml_amd.mf import MFbasemode
    monkeypatch.setattr(driver, "_default_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(driver, "_make_engine", lambda dev, d, mb: _CpuEngine(dev, d, mb))
    monkeypatch.setattr(MFbasemode, "test", _cpu_mf_test)
    meta, log, flat, z = run_g12(tmp_path, teacher_forced=True)
    assert meta._forced_stages == [2, 3]
    want = str(z["log"])
    norm = lambda t: [" ".join(l.split()) for l in t.splitlines() if "time cost" not in l and "is:" not in l]
    assert [_NUM.sub("#", l) for l in norm(log)] == [_NUM.sub("#", l) for l in norm(want)]      # same text, line by line
    r = g12_compare(log, want, flat, z, stages=(0, 2, 3), loss_rtol=1e-4, flips=2)
    free = g12_compare(log, want, flat, z, stages=(1,), loss_rtol=1.0, flips=10000)
    print("G12 oracle: teacher-forced/seeded stages: loss rel %.2e recall %.4f ndcg %.4f | free-running stage 1: "
          "loss rel %.2e recall %.4f ndcg %.4f" % (r + free))


def g15_compare(log, want_log, flat, z, tight_phases=10, loss_rtol=1e-4, flips=2, late_rtol=3e-3, late_flips=8):
    """G15 against the reference, stage by stage and PHASE by phase (multi_num = 10 phases per stage).  Held: the per-batch
    losses within loss_rtol and the printed Recall@20 / NDCG@20 within `flips` rank flips on phases [0, tight_phases) of every
    stage, late_rtol / late_flips on the rest (a free-running comparison uses tight_phases = 0: trajectories of a chaotic loop
    that started 1e-7 apart are 1e-4 apart a few hundred transfer steps later -- measured, profiles/r05_parity_g15_*.json).
    The whole picture is RETURNED: {stage: {"loss_rel_by_phase": [...], "recall_diff_by_phase": [...], "ndcg_diff_by_phase": [...]}}."""
    tags, ref = z["batch_tag"], z["batch_loss"]
    P = int(z["config"][8])
    assert len(flat) == len(ref) and all((a[0], a[1]) == (int(t[0]), int(t[1])) for a, t in zip(flat, tags))
    got = np.array([a[2] for a in flat])
    rel = np.abs(got - ref) / np.abs(ref)

    def blocks(text):
        out, cur = [], None
        for l in text.splitlines():
            if l.startswith("now time:") and (cur is None or not cur[-1].startswith("now time:")) \
                    and (cur is None or not cur[-1].startswith("will be test")):
                if cur is not None and any("MF (inner)" in x for x in cur):
                    out.append(cur)
                    cur = []
                elif cur is None:
                    cur = []
            if cur is not None:
                cur.append(l)
        out.append(cur)
        return out
    gb, wb = blocks(log), blocks(want_log)
    n_stage = int(tags[:, 0].max()) + 1
    assert len(gb) == len(wb) == n_stage, (len(gb), len(wb))
    n_rows = float(z["test_num"][0])
    rep = {}
    for st in range(n_stage):
        lr = np.zeros(P)
        for kind in (0, 1):
            r = rel[(tags[:, 0] == st) & (tags[:, 1] == kind)]
            per = r.size // P
            assert per * P == r.size
            lr = np.maximum(lr, r.reshape(P, per).max(1))
        # a phase = the lines from one "MF (inner) training" banner to the next (a test stage's "test result" lines sit inside
        # phase 0: the reference tests the incoming period after the first MF epoch)
        def phases(lines):
            out = []
            for l in lines:
                if "MF (inner)" in l:
                    out.append([])
                if out:
                    out[-1].append(l)
            return [g12_losses_from_log("\n".join(p_)) for p_ in out]
        g, w = phases(gb[st]), phases(wb[st])
        assert len(g) == len(w) == P, (len(g), len(w))
        dr, dn = np.zeros(P), np.zeros(P)
        for ph in range(P):
            assert [x[0] for x in g[ph]] == [x[0] for x in w[ph]]
            for (k, a, _), (_, b, _) in zip(g[ph], w[ph]):
                if k == "recall":
                    dr[ph] = max(dr[ph], abs(a - b))
                elif k == "ndcg":
                    dn[ph] = max(dn[ph], abs(a - b))
        head = 0.0
        rep[st] = {"loss_rel_by_phase": [float(x) for x in lr], "recall_diff_by_phase": [float(x) for x in dr],
                   "ndcg_diff_by_phase": [float(x) for x in dn], "test_lines_max_diff": float(head)}
        T = tight_phases
        if T == 0:
            lr_t = dr_t = dn_t = np.zeros(1)
        else:
            lr_t, dr_t, dn_t = lr[:T], dr[:T], dn[:T]
        assert lr_t.max() <= loss_rtol, "stage %d: per-batch loss rel err %.2e in phases < %d" % (st, lr_t.max(), T)
        assert lr.max() <= late_rtol, "stage %d: per-batch loss rel err %.2e" % (st, lr.max())
        assert dr_t.max() <= flips / n_rows + 1e-9 and dn_t.max() <= flips / n_rows + 0.5e-4 + 1e-9, (st, dr, dn)
        assert dr.max() <= late_flips / n_rows + 1e-9 and dn.max() <= late_flips / n_rows + 0.5e-4 + 1e-9, (st, dr, dn)
        assert head <= flips / n_rows + 0.5e-4 + 1e-9, (st, head)
    return rep


def test_g15_full_depth_sequence_on_cpu_oracle(tmp_path, monkeypatch):
    """G15 (round 5): the reference's period loop at its DEFAULT depth -- multi_num 10 -- over 6 stages, 4 of them
    test stages, 10,000 test rows each (one rank flip = 1e-4), state snapshots at EVERY stage start.  The oracle through the
    product's driver, teacher-forced at every stage (the forcing is asserted to have happened): same text line by line; every
    per-batch loss -- 3,000 of them, ten phases deep into every stage -- within 1e-4 of the scalar the reference backpropagated
    (measured: 1e-7 in the forced stages, 5e-5 in stage 0, which starts from the seeds), every printed Recall@20 / NDCG@20
    within 2 rank flips."""
    from sml_amd import driver
    from sml_amd.mf import MFbasemode
    monkeypatch.setattr(driver, "_default_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(driver, "_make_engine", lambda dev, d, mb: _CpuEngine(dev, d, mb))
    monkeypatch.setattr(MFbasemode, "test", _cpu_mf_test)
    meta, log, flat, z = run_g12(tmp_path, teacher_forced=True, name="g15_fulldepth")
    assert meta._forced_stages == [1, 2, 3, 4, 5]
    want = str(z["log"])
    norm = lambda t: [" ".join(l.split()) for l in t.splitlines() if "time cost" not in l and "is:" not in l]
    assert [_NUM.sub("#", l) for l in norm(log)] == [_NUM.sub("#", l) for l in norm(want)]
    assert len(flat) == 3000 and int(z["config"][8]) == 10
    rep = g15_compare(log, want, flat, z)
    print("G15 oracle, teacher-forced at every stage; worst per-batch loss rel err by phase, per stage:")
    for st, r in rep.items():
        print("  stage %d:" % st, " ".join("%.1e" % v for v in r["loss_rel_by_phase"]), "| recall", max(r["recall_diff_by_phase"]))


def _g10_stream(g):
    """The tiny stream G10 was recorded on (tests/golden/make_golden.py: gen_g10)."""
    U, I, n_train, n_test, neg = 80, 60, 700, 90, 49
    rng = np.random.RandomState(31)
    train = np.stack([rng.randint(0, U, n_train), rng.randint(0, I, n_train)], 1).astype(np.int64)
    test = np.zeros((n_test, 2 + neg), dtype=np.int64)
    for r in range(n_test):
        test[r, 0] = rng.randint(0, U)
        test[r, 1] = rng.randint(0, I)
        test[r, 2:] = rng.choice(np.setdiff1d(np.arange(I), [test[r, 1]]), size=neg, replace=False)
    assert np.array_equal(test, g["test_rows"])

    class Stream(object):
        test_new_user = np.zeros(0, dtype=np.int64)
        test_new_item = np.zeros(0, dtype=np.int64)

        def get_next(self, stage_id, types="not_only_new"):
            return train, test
    return Stream(), U, I


def run_g10_finetune(engine, device):
    """model.baseline.SPMF.run_one_stage2 under the seeds G10 was recorded with; returns (spmf, log, batches)."""
    import contextlib
    import io
    import types
    from model.baseline import SPMF
    g = golden("g10_baseline_adam.npz")
    stream, U, I = _g10_stream(g)
    args = types.SimpleNamespace(lr=0.01, pool_size=0, neg_num=1, batch_size=128, l2_u=1e-5, l2_i=1e-5, epochs=3,
                                 pool_init_type=0)
    seen = []
    real = engine.bare_adam_epoch

    def spy(mf, triples, *a, **k):
        seen.append(np.asarray(triples).copy())
        return real(mf, triples, *a, **k)
    engine.bare_adam_epoch = spy
    torch.manual_seed(41)
    np.random.seed(42)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        sp = SPMF(args, stream, U, I, 32, device=device, engine=engine)
        with torch.no_grad():
            sp.MFbase.user_laten.weight.mul_(0.3)
            sp.MFbase.item_laten.weight.mul_(0.3)
        assert sp.run_one_stage2(1, read_data_type="only_new")
    return g, sp, buf.getvalue(), seen


def test_baseline_finetune_loop_replays_reference_batches_and_log():
    """G10 through the product's model.baseline.SPMF with the oracle injected as the engine: the batches
    (DataLoader shuffle + per-item negative sampling streams), the printed epoch losses and the final
    recall/ndcg are the reference's."""
    from _cpu_engine import CpuEngine
    eng = CpuEngine(d=32)
    eng.mf_forward = lambda wu, wi, u, i, norm=False: O.mf_forward(wu, wi, u, i, norm)
    g, sp, log, seen = run_g10_finetune(eng, "cpu")
    assert len(seen) == 3
    for e in range(3):
        assert np.array_equal(seen[e], g["triples_%d" % e])
    losses = [float(l.split("loss:")[1]) for l in log.splitlines() if l.startswith("epoch:")]
    np.testing.assert_allclose(losses, g["epoch_loss"], atol=1.01e-4)
    np.testing.assert_allclose(sp.recall[-1], g["recall_5_10_20"], atol=1e-9)
    np.testing.assert_allclose(sp.ndcg[-1], g["ndcg_5_10_20"], atol=1e-5)
    assert "before train test---" in log and "FInal test---" in log and "max result " in log


def test_csr_resolver_equals_pair_list_resolver():
    """sml_host_resolve_negatives_csr (two memory touches per candidate) walks the candidate stream exactly as
    sml_host_resolve_negatives (bisection of the sorted pair list) does: same negatives, same consumption, also
    when the stream runs out mid-element and for users with long item lists."""
    from sml_amd import _lib
    lib = _lib.load()
    rng = np.random.RandomState(9)
    U, I, n_pairs = 40, 30, 500
    pairs = np.unique(rng.randint(0, U, n_pairs).astype(np.int64) * I + rng.randint(0, I, n_pairs))
    pu = pairs // I
    uptr = np.ascontiguousarray(np.searchsorted(pu, np.arange(U + 1)), dtype=np.int64)
    uitems = np.ascontiguousarray(pairs % I, dtype=np.int64)
    for n, m in ((200, 200), (200, 120), (1, 1), (64, 1000)):
        users = np.ascontiguousarray(rng.randint(0, U, n), dtype=np.int64)
        cand = np.ascontiguousarray(rng.randint(0, I, m), dtype=np.int64)
        out = []
        for fn, extra in ((lib.sml_host_resolve_negatives, (pairs.ctypes.data, pairs.shape[0], I)),
                          (lib.sml_host_resolve_negatives_csr, (uptr.ctypes.data, U, uitems.ctypes.data))):
            negs = np.full(n, -7, dtype=np.int64)
            used, got = ctypes.c_int64(0), ctypes.c_int64(0)
            rc = fn(users.ctypes.data, n, cand.ctypes.data, m, *extra, negs.ctypes.data, ctypes.byref(used), ctypes.byref(got))
            assert rc == 0
            out.append((negs[:got.value].copy(), used.value, got.value))
        assert out[0][1:] == out[1][1:]
        assert np.array_equal(out[0][0], out[1][0])
        own = set(pairs.tolist())
        assert all(int(u) * I + int(c) not in own for u, c in zip(users[:out[1][2]], out[1][0]))


# ----------------------------------------------------------------------------- multi-GPU set-up logic (no GPU involved)
class _FakePeerEngine(object):
    """The part of HipEngine's surface sml_amd.dist._PeerSetup uses, with a scripted outcome per step."""
    device = torch.device("cpu")

    def __init__(self, kind=0, fail_at=None):
        self.kind, self.fail_at, self.calls, self.freed, self.closed = kind, fail_at, [], [], []

    def _step(self, name):
        self.calls.append(name)
        if self.fail_at == name:
            raise RuntimeError("scripted failure in %s" % name)

    def peer_region_bytes(self, world, rows_cap):
        return 64, 64

    def peer_alloc(self, nbytes):
        self._step("alloc")
        return 0x1000 + 0x100 * len([c for c in self.calls if c == "alloc"])

    def peer_mem_kind(self, ptr):
        return self.kind

    def peer_export(self, ptr):
        self._step("export")
        return b"h" * 64

    def peer_open(self, handle):
        self._step("open")
        return 0x9000 + len(self.calls)

    def peer_attach(self, *a, **k):
        self._step("attach")

    def peer_allreduce_check(self, src, timeout_s=0.0):
        self._step("check")
        return src * 0.0            # never the expected sum: the self-check fails

    def peer_status(self):
        return 0

    def peer_detach(self):
        self.calls.append("detach")

    def peer_close(self, ptr):
        self.closed.append(ptr)

    def peer_free(self, ptr):
        self.freed.append(ptr)


@pytest.mark.parametrize("case", ["plain_across_devices", "one_rank_fails_to_open", "self_check_fails"])
def test_peer_setup_leaves_a_failing_path_on_every_rank_together_and_releases_its_regions(case, monkeypatch):
    """sml_amd.dist.peer_setup: every local step is followed by an all-ranks vote, so a rank that fails
    alone does not leave its peers in a mismatched collective; plain (coarse-grained) inbox memory is REFUSED when the
    ranks sit on different devices; whatever the set-up allocated or mapped is released on the way out."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from _thread_group import run_ranks
    from sml_amd import dist as SD
    monkeypatch.setattr(SD, "_device_identity", lambda e: ("host", e.rank_tag))

    class Procs(object):              # a 2-rank group that does NOT look like threads of one process: handles travel
        def __init__(self, g):
            self.g = g

        def __getattr__(self, k):
            return getattr(self.g, k)

        def get_backend(self, group=None):
            return "gloo"

    def rank_fn(rank, group):
        e = _FakePeerEngine(kind=2 if case == "plain_across_devices" else 0,
                            fail_at="open" if case == "one_rank_fails_to_open" and rank == 1 else None)
        e.rank_tag = rank             # two different devices
        ok = SD.peer_setup(e, Procs(group), None, rows_cap=8, timeout_s=1.0)
        return ok, e

    (ok0, e0), (ok1, e1) = run_ranks(2, rank_fn)
    assert ok0 is False and ok1 is False
    for e in (e0, e1):
        assert "detach" in e.calls and len(e.freed) == 2          # inbox + flags given back
    if case == "plain_across_devices":
        assert "export" not in e0.calls and "attach" not in e0.calls      # refused before anything is mapped
    if case == "one_rank_fails_to_open":
        assert "attach" not in e0.calls and "attach" not in e1.calls       # rank 0 opened fine, and still left with rank 1
        assert len(e0.closed) == 2
    if case == "self_check_fails":
        assert e0.calls.count("check") >= 2 and len(e0.closed) == 2


@pytest.mark.parametrize("case", ["all_fine", "one_rank_fails_to_open", "stale_read"])
def test_shard_visibility_check_releases_mappings_and_probe_on_every_path(case):
    """sml_amd.dist.shard_visibility_check: whichever vote ends it -- an open that failed on one rank, a stale
    read, or success -- every rank closes the mappings it opened and frees its probe allocation, all ranks together."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from _thread_group import run_ranks
    from sml_amd import dist as SD

    class Procs(object):
        def __init__(self, g):
            self.g = g

        def __getattr__(self, k):
            return getattr(self.g, k)

        def get_backend(self, group=None):
            return "gloo"

    class Eng(_FakePeerEngine):
        def __init__(self, rank, **kw):
            super().__init__(**kw)
            self.rank, self.probe, self.freed_probes = rank, None, 0

        def peer_tensor(self, shape, dtype=torch.float32):
            self.probe = torch.zeros(shape, dtype=dtype)
            return self.probe

        def peer_tensor_free(self, t):
            assert t is self.probe
            self.freed_probes += 1

        def peer_export(self, ptr):
            return ("probe of rank %d" % self.rank).encode().ljust(64, b" ")

        def peer_open(self, handle):
            self._step("open")
            return 0x9000 + int(handle.decode().split()[3])           # "address" that names the owner rank

        def peer_read(self, ptr, n):
            owner = ptr - 0x9000 if 0x9000 <= ptr < 0x9100 else self.rank
            t = BOARD[owner].clone()
            return t * 0 if (case == "stale_read" and self.rank == 1 and owner == 0) else t

    BOARD = {}
    monkey = torch.cuda.synchronize
    torch.cuda.synchronize = lambda *a, **k: None
    try:
        def rank_fn(rank, group):
            e = Eng(rank, fail_at="open" if case == "one_rank_fails_to_open" and rank == 1 else None)
            orig = e.peer_tensor

            def tracked(shape, dtype=torch.float32):
                t = orig(shape, dtype)
                BOARD[rank] = t
                return t
            e.peer_tensor = tracked
            return SD.shard_visibility_check(e, Procs(group), None, rounds=2, n=64), e
        (ok0, e0), (ok1, e1) = run_ranks(2, rank_fn)
    finally:
        torch.cuda.synchronize = monkey
    assert ok0 is ok1 is (case == "all_fine")
    assert e0.freed_probes == 1 and e1.freed_probes == 1
    assert len(e0.closed) == 1 and len(e1.closed) == (0 if case == "one_rank_fails_to_open" else 1)


def test_check_exchange_fingerprints_stay_exact_above_2_to_the_53():
    """DistContext.check_exchange: the bit fingerprints travel as int64 -- a float64 cast cannot tell two sums
    above 2^53 that differ by one."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from _thread_group import run_ranks
    from sml_amd import dist as SD

    def rank_fn(rank, group):
        ctx = SD.DistContext(group, torch.device("cpu"))
        ctx.mode = "torch"
        big = torch.full((1 << 23,), 2.0 ** 31 - 1, dtype=torch.float32)       # bit pattern 0x4f000000: the sum passes 2^53
        x = big.clone()
        ctx.check_exchange(None, "equal replicas", replicas=[x])
        if rank == 1:
            x[5] = torch.tensor([x[5]]).view(torch.int32).add(1).view(torch.float32)[0]     # one ulp on one rank
        try:
            ctx.check_exchange(None, "one ulp apart", replicas=[x])
        except RuntimeError as e:
            return "differ" in str(e)
        return False
    assert run_ranks(2, rank_fn) == [True, True]


def test_product_library_has_no_library_sort():
    """the hipCUB radix-sort path of the index preparation is a test-only reference (tests/csrc, compiled into
    tests/_ref/libsml_hip_prepref.so by tests/build_reference.py).  The product library carries no hipcub / rocprim symbol and
    its sources reach that code only under -DSML_TEST_PREP_REFERENCE."""
    import subprocess
    from sml_amd import _lib, build
    out = subprocess.run(["nm", "-C", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "hipcub" not in out and "rocprim" not in out
    for src in build.SOURCES:
        text = open(os.path.join(build.CSRC, src)).read()
        depth, guarded = 0, True
        for line in text.splitlines():
            t = line.strip()
            if t.startswith("#ifdef SML_TEST_PREP_REFERENCE"):
                depth += 1
            elif t.startswith("#endif") and depth:
                depth -= 1
            elif ("hipcub" in t or "tests/csrc" in t) and not t.startswith("//") and depth == 0:
                guarded = False
        assert guarded, src


def test_no_kernel_spills_or_uses_scratch_memory():
    """Round 6: several kernels patch a local copy of (part of) their by-value argument struct with preloaded parameters; a copy
    that is indexed dynamically anywhere cannot live in registers and lands in scratch memory (560 bytes per lane in the first attempt
    at k_transfer_bwd_full) -- slow, and silent.  The compiler's resource remarks for every kernel of transfer_net.hip / mf_kernels.hip
    with the product's flags: no spilled VGPR, no scratch (tools/kernel_resources.py; hipcc cross-compiles without a GPU).

    The same report pins the instantiation sets of the transfer net's forward and MF backward: every form has a launch site that some
    input reaches by default, the TR stage's backward is k_tr_bwd_head + k_tr_wgrad2 alone (no TR flag on the MF kernels, no
    k_transfer_wgrad), and a form that only a switch could select does not come back unnoticed."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(repo, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    names = {line.split("  ")[0] for line in p.stdout.splitlines()}
    assert "k_tr_wgrad2<32>" in names and "k_tr_bwd_head<32>" in names                              # (the report really covered the kernels)

    def family(k):
        return {n for n in names if n.startswith(k + "<")}
    fwd = {"k_transfer_fwd<%d, 1, %d, 1>" % (d, ns) for d in (32, 64, 128) for ns in (1, 2, 4)}
    fwd |= {"k_transfer_fwd<32, 2, 1, 2>", "k_transfer_fwd<64, 2, 1, 2>", "k_transfer_fwd<128, 2, 1, 1>"}
    assert family("k_transfer_fwd") == fwd, sorted(family("k_transfer_fwd") ^ fwd)
    bwd = {"k_transfer_bwd<32, true>", "k_transfer_bwd<64, false>", "k_transfer_bwd<128, false>"}     # <D, PRE>
    assert family("k_transfer_bwd") == bwd, sorted(family("k_transfer_bwd") ^ bwd)
    full = {"k_transfer_bwd_full<%d, 1>" % d for d in (32, 64, 128)}
    assert family("k_transfer_bwd_full") == full, sorted(family("k_transfer_bwd_full") ^ full)
    assert not [n for n in names if "k_transfer_wgrad" in n]


def test_tr_with_mf_bias_fails_like_the_reference_does(tmp_path, monkeypatch):
    """--TR_with_MF_bias (model/transfer.py:347-354): the reference gives W_{t-1} d + 1 columns and then multiplies it with d-column MF
    rows in ConvTransfer_com.forward (model/conv_transfer.py:93) -- run here on the reference itself (round 5): RuntimeError "The size of
    tensor a (33) must match the size of tensor b (32) at non-singleton dimension 1" in the first MF batch.  The product raises the same
    error type with the same sizes, up front."""
    from sml_amd import cli, datasets, driver, synth
    from sml_amd.mf import MFbasemode
    monkeypatch.setattr(driver, "_default_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(driver, "_make_engine", lambda dev, d, mb: _CpuEngine(dev, d, mb))
    root = str(tmp_path) + "/"
    synth.write_dataset(root, "yelp", n_periods=4, n_inter=300, n_user=60, n_item=40, neg=9, seed=7)
    torch.manual_seed(1)
    ck = os.path.join(root, "init.pkl")
    torch.save(MFbasemode(60, 40, 32), ck)
    args = cli.get_parse("yelp").parse_args(["--data_path", root, "--pre_model", ck, "--laten", "32", "--numworkers", "0", "--TR_with_MF_bias", "True"])
    with quiet():
        sets = datasets.transfer_data(args, path=root, datasetname="yelp", file_path_list=["0", "1", "2", "3"], test_list=["2", "3"],
                                      validation_list=None, online_train_time=1, online_test_time=2)
        with pytest.raises(RuntimeError, match=r"size of tensor a \(33\) must match the size of tensor b \(32\)"):
            driver.meta_train(args, sets, sets.user_number, sets.item_number, args.laten)


def test_zipf_head_rows_of_the_sharded_bare_step():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_head", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.zipf_head_rows(1000000, 0.0, 1 << 22, 64, 197000) == 0            # uniform catalogue: nothing to replicate
    h = bench.zipf_head_rows(1000000, 1.0, 8 * 2 * 262144, 64, 197000)
    assert 0 < h <= 2 * 197000 // 64 and h % 4 == 0                                # capped by the dense partial's slot
    small = bench.zipf_head_rows(1000000, 1.0, 2 * 4096, 32, 98943)
    assert 0 < small < 100                                                         # few rows reach 16 occurrences of 8,192


def test_bench_dump_outputs_keeps_a_fixed_sample_under_64_mb(tmp_path):
    """bench.py --dump-outputs: float32 .npy files, whole when they fit, otherwise the same seeded rows of every table in
    every run, and never more than 64 MB in all."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_dump", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    g = torch.Generator().manual_seed(0)
    loss, wu, wi = torch.rand(16, generator=g), torch.rand(1000000, 32, generator=g), torch.rand(300000, 32, generator=g).half()
    small = tmp_path / "small"
    bench.dump_outputs(str(small), [("loss", loss), ("absent", None), ("item_emb", wi[:1000])])
    assert sorted(os.listdir(str(small))) == ["item_emb.npy", "loss.npy"]
    np.testing.assert_array_equal(np.load(str(small / "item_emb.npy")), wi[:1000].float().numpy())
    runs = []
    for r in range(2):
        d = tmp_path / ("big%d" % r)
        bench.dump_outputs(str(d), [("loss", loss), ("user_emb", wu), ("item_emb", wi)])
        assert sum(os.path.getsize(str(d / f)) for f in os.listdir(str(d))) <= 64 * 10 ** 6
        runs.append({f: np.load(str(d / f)) for f in os.listdir(str(d))})
    assert all(v.dtype == np.float32 for v in runs[0].values())
    assert 0 < runs[0]["user_emb.npy"].shape[0] < wu.shape[0] and 0 < runs[0]["item_emb.npy"].shape[0] < wi.shape[0]
    np.testing.assert_array_equal(runs[0]["loss.npy"], loss.numpy())
    for f in runs[0]:
        np.testing.assert_array_equal(runs[0][f], runs[1][f])
    where = {r.tobytes(): k for k, r in enumerate(wu.numpy())}
    rows = [where[r.tobytes()] for r in runs[0]["user_emb.npy"]]          # (KeyError: not a row of the table)
    assert all(a < b for a, b in zip(rows, rows[1:]))                      # distinct rows, in table order
