"""SPMF on the MI355X: sml_rank_weights (scores, stable device radix sort, p), sml_weighted_epoch, the stream-exact SPMF
stage against fixture G16, and the `model.baseline` command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from test_spmf_host import _ulp_diff, g16, run_g16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def engine(d):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tables(d, n_user, n_item, seed=0):
    rng = np.random.RandomState(seed)
    return (rng.randn(n_user, d).astype(np.float32) * 0.3, rng.randn(n_item, d).astype(np.float32) * 0.3)


def numpy_order(score):
    """torch.argsort(descending=True, stable=True) on CPU: NaN first, -0.0 == +0.0, ties by row index."""
    s = score.astype(np.float64)
    nan = np.isnan(s)
    return np.lexsort((np.arange(s.shape[0]), np.where(nan, 0.0, -s) + 0.0, np.where(nan, 0, 1)))


def test_numpy_order_matches_torch_cpu():
    s = np.array([1, np.nan, -0.0, 0.0, 2], dtype=np.float32)
    assert numpy_order(s).tolist() == [1, 4, 0, 2, 3] == torch.argsort(torch.from_numpy(s), descending=True, stable=True).tolist()


def p_formula(rank, n):
    """w = exp(float32(rank) / float32(n)) correctly rounded to float32, S = float32(float64 sum of all w), p = w / S."""
    x = (rank.astype(np.float32) / np.float32(n)).astype(np.float32)
    w = np.exp(x.astype(np.float64)).astype(np.float32)
    xs = (np.arange(1, n + 1, dtype=np.float64).astype(np.float32) / np.float32(n)).astype(np.float32)
    S = np.float32(np.exp(xs.astype(np.float64)).astype(np.float32).astype(np.float64).sum())
    return (w / S).astype(np.float32)


def check_rank_weights(eng, wu, wi, rows, planted=None):
    wu_d, wi_d = gpu(wu), gpu(wi)
    rows_d = gpu(rows)
    score, rank, order, p = eng.rank_weights(wu_d, wi_d, rows_d)
    _, _, ref_score = eng.mf_forward(wu_d, wi_d, rows_d[:, 0].contiguous(), rows_d[:, 1].contiguous())
    score, rank, order, p = (t.cpu().numpy() for t in (score, rank, order, p))
    assert score.tobytes() == ref_score.cpu().numpy().tobytes()
    n = rows.shape[0]
    want = numpy_order(score)
    assert np.array_equal(order, want)
    inv = np.empty(n, np.int64)
    inv[order] = np.arange(1, n + 1)
    assert np.array_equal(rank, inv)
    _, _, _, p2 = eng.rank_weights(wu_d, wi_d, rows_d)
    assert p.tobytes() == p2.cpu().numpy().tobytes()
    assert _ulp_diff(p, p_formula(rank, n)).max() <= 2
    assert abs(p.astype(np.float64).sum() - 1.0) <= 1e-6
    return score, order


@pytest.mark.parametrize("d", [32, 64, 128])
def test_rank_weights_random_and_planted(d):
    eng = engine(d)
    wu, wi = tables(d, 300, 200, seed=d)
    rng = np.random.RandomState(d)
    for n in (1, 7, 4095, 4096, 4097, 70001):
        rows = np.stack([rng.randint(0, 300, n), rng.randint(0, 200, n)], 1).astype(np.int64)
        if n > 10:
            rows[n // 2:n // 2 + 50] = rows[3]                   # planted ties: the same row many times
        check_rank_weights(eng, wu, wi, rows)


def test_rank_weights_signed_zero_nan_all_equal():
    eng = engine(32)
    wu, wi = tables(32, 8, 8, seed=1)
    wu[0] = 0.0                                                    # user 0 scores +0.0 with anything
    wu[1] = -0.0
    wi[0] = 0.0
    wu[2, 0] = np.nan                                              # user 2 scores NaN
    wu[3] = np.inf                                                 # inf * mixed signs -> NaN or +-inf
    rows = np.array([[u, i] for u in range(8) for i in range(8)] * 3, dtype=np.int64)
    score, order = check_rank_weights(eng, wu, wi, rows)
    assert np.isnan(score).any() and (score == 0).any()
    same = np.zeros((10000, 2), dtype=np.int64)                    # all equal
    _, order = check_rank_weights(eng, wu, wi, same)
    assert np.array_equal(order, np.arange(10000))


def test_rank_weights_beyond_fp32_rank():
    """N = 2^24 + 3: (float)rank rounds; p follows the stated formula and sums to 1."""
    eng = engine(32)
    wu, wi = tables(32, 1000, 1000, seed=5)
    rng = np.random.RandomState(5)
    n = (1 << 24) + 3
    rows = np.stack([rng.randint(0, 1000, n), rng.randint(0, 1000, n)], 1).astype(np.int64)
    check_rank_weights(eng, wu, wi, rows)


def _epoch_setup(n=3000, seed=11):
    rng = np.random.RandomState(seed)
    rows = np.stack([rng.randint(0, 80, n), rng.randint(0, 60, n)], 1).astype(np.int64)
    codes = np.unique(rows[:, 0] * 60 + rows[:, 1])
    ptr = np.searchsorted(codes // 60, np.arange(81)).astype(np.int64)
    items = (codes % 60).astype(np.int64)
    item_all = np.unique(rows[:, 1])
    return rows, codes, ptr, items, item_all


def test_weighted_epoch_valid_reproducible_and_distributed():
    eng = engine(32)
    wu, wi = tables(32, 80, 60, seed=2)
    rows, codes, ptr, items, item_all = _epoch_setup()
    n = rows.shape[0]
    _, rank, order, p = eng.rank_weights(gpu(wu), gpu(wi), gpu(rows))
    m = 2_000_000
    tri, failed = eng.weighted_epoch(gpu(rows), order, gpu(item_all), gpu(ptr), gpu(items), m, 1234)
    tri2, _ = eng.weighted_epoch(gpu(rows), order, gpu(item_all), gpu(ptr), gpu(items), m, 1234)
    tri3, _ = eng.weighted_epoch(gpu(rows), order, gpu(item_all), gpu(ptr), gpu(items), m, 1235)
    tri, tri2, tri3 = tri.cpu().numpy(), tri2.cpu().numpy(), tri3.cpu().numpy()
    assert int(failed[0]) == 0
    assert np.array_equal(tri, tri2) and not np.array_equal(tri, tri3)
    assert np.isin(tri[:, 0] * 60 + tri[:, 1], codes).all()                   # every (u, i) is a training row
    assert not np.isin(tri[:, 0] * 60 + tri[:, 2], codes).any()               # no negative is one of the user's items
    assert np.isin(tri[:, 2], item_all).all()
    # rank deciles: the row's rank through its (u, i) code (rows may repeat: count by code)
    rank = rank.cpu().numpy()
    p = p.cpu().numpy().astype(np.float64)
    code_of_row = rows[:, 0] * 60 + rows[:, 1]
    uc, inv = np.unique(code_of_row, return_inverse=True)
    p_code = np.bincount(inv, weights=p, minlength=uc.shape[0])
    got = np.bincount(np.searchsorted(uc, tri[:, 0] * 60 + tri[:, 1]), minlength=uc.shape[0])
    exp = p_code / p_code.sum() * m
    chi = ((got - exp) ** 2 / exp).sum()
    dof = uc.shape[0] - 1
    assert chi < dof + 6 * np.sqrt(2 * dof), (chi, dof)
    # deciles of rank, by the expected mass of each decile (a row with copies counted at each copy's rank share)
    dec = np.minimum((rank - 1) * 10 // n, 9)
    exp_d = np.bincount(dec, weights=p, minlength=10) * m
    share = p / p_code[inv]
    got_d = np.bincount(dec, weights=got[inv] * share, minlength=10)
    chi_d = ((got_d - exp_d) ** 2 / exp_d).sum()
    assert chi_d < 9 + 6 * np.sqrt(18), chi_d


def test_weighted_epoch_counts_failures():
    eng = engine(32)
    rows = np.array([[0, 1], [0, 2], [1, 3]], dtype=np.int64)
    ptr = np.array([0, 2, 3], dtype=np.int64)
    items = np.array([1, 2, 3], dtype=np.int64)
    item_all = np.array([1, 2], dtype=np.int64)                    # user 0 owns every item of the period
    order = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    tri, failed = eng.weighted_epoch(gpu(rows), order, gpu(item_all), gpu(ptr), gpu(items), 5000, 3)
    tri = tri.cpu().numpy()
    assert int(failed[0]) == int((tri[:, 0] == 0).sum()) > 0
    assert np.isin(tri[:, 2], item_all).all()


@pytest.mark.parametrize("ptype", [0, 1])
def test_spmf_stage_on_gpu_against_g16(ptype, tmp_path):
    """The stream-exact SPMF run on the HIP engine (device rank weights, HIP bare step, rank-kernel evaluation).
    Stage 2 ranks the initial tables: the device p is G16's up to the order of copies of one row, which the
    reference's argsort ranks either way (|delta cdf| < 1e-4; the uniforms within that distance of a bin edge are
    counted and at most 4 of the first batch's 64).  Every stage then samples with G16's p, so the batches are G16's bit for bit and the losses,
    metrics and log match at the host test's tolerances: the HIP path end to end, free of the ranking of tied copies."""
    from sml_amd.engine import HipEngine
    from test_spmf_host import check_g16_run
    eng = HipEngine(DEV, 32, 4096)                 # fresh: the MF Adam state (m, v, step) starts at zero as torch's does
    seen, ps = [], []
    real_bare, real_rw = eng.bare_adam_epoch, eng.rank_weights
    g = g16()
    pre = "t%d." % ptype
    ref_ps = [g[pre + "p0"], g[pre + "p1"]]

    def spy(mf, triples, *a, **k):
        seen.append(np.asarray(triples.cpu() if isinstance(triples, torch.Tensor) else triples).copy())
        return real_bare(mf, triples, *a, **k)

    def rw(*a, **k):
        out = real_rw(*a, **k)
        ps.append(out[3].cpu().numpy())
        return out[:3] + (torch.from_numpy(ref_ps[len(ps) - 1]),)
    eng.bare_adam_epoch, eng.rank_weights = spy, rw
    g, sp, log = run_g16(ptype, eng, tmp_path, device=DEV)
    cdf = lambda a: np.cumsum(a.astype(np.float64)) / a.astype(np.float64).sum()
    c_dev, c_ref = cdf(ps[0]), cdf(ref_ps[0])
    gap = np.abs(c_dev - c_ref)
    assert gap.max() < 1e-4
    # the stage's uniforms, replayed: the generator state at the start of stage 2 is where base_train_not_train left it
    np.random.seed(2002)
    from sml_amd.baseline import Reservious
    import contextlib
    import io
    train, _ = __import__("test_spmf_host").g16_stream()
    with contextlib.redirect_stdout(io.StringIO()):
        r = Reservious(g["hyper"][5].astype(int))
    (r.init_pool if ptype == 1 else r.updata)(train[0])
    u = np.random.random_sample(64)                         # the first batch's uniforms
    near = int((np.abs(c_ref[None, :] - u[:, None]) <= gap[None, :]).any(axis=1).sum())
    assert near <= 4, near
    check_g16_run(g, sp, log, seen, ptype)


def _cli(tmp_path, *extra):
    from sml_amd import synth
    root = str(tmp_path)
    synth.write_dataset(root, "tiny", 4, 400, 70, 60, neg=30, seed=7)
    np.save(os.path.join(root, "tiny", "test_new_user.npy"), np.arange(0, 70, 9, dtype=np.int64))
    np.save(os.path.join(root, "tiny", "test_new_item.npy"), np.arange(0, 60, 7, dtype=np.int64))
    cmd = [sys.executable, "-m", "model.baseline", "--data_path", root + "/", "--data_name", "tiny", "--pre_model", "",
           "--start_idx", "2", "--epochs", "3", "--batch_size", "64", "--laten_dim", "32", "--pool_size", "300"] + list(extra)
    r = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-3000:]
    assert "weight average recall@20:" in out and "weight average ndcg@20:" in out and "last 7 (test) results" in out, out[-3000:]
    assert out.count("#################################runing stage:") == 3      # stages 2, 3 and the end of the data
    return out


@pytest.mark.parametrize("method", ["spmf", "full", "fine"])
def test_cli_methods_run_on_synthetic_data(method, tmp_path):
    _cli(tmp_path, "--method", method)


def test_cli_spmf_device_batches(tmp_path):
    out = _cli(tmp_path, "--method", "spmf", "--device_batches", "1", "--lr", "0.002")
    losses = [float(l.split("loss:")[1]) for l in out.splitlines() if l.startswith("epoch:")]
    assert len(losses) == 6 and np.isfinite(losses).all()
    for s in range(2):
        e = losses[3 * s:3 * s + 3]
        assert e[2] < e[0], losses
