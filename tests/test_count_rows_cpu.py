"""CPU-only checks of the per-query thresholds and the k-th neighbour search (select_kth_rows, eps_to_ssd_rows, density_ratio_loss, the
argument refusals of kth_distances / ball_counts_rows / attack_models.density): the host search against np.sort, the vectorised thresholds
against eps_to_ssd value by value, and every refusal that must come before a GPU is touched."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bound(s_max):
    p, reach = 0, 1
    while reach < s_max + 2:
        p, reach = p + 1, reach * 17
    return p


def _count_fn(rows, log=None):
    """count_fn of select_kth_rows over a list of sorted int64 multisets; also checks what the search may assume of its thresholds"""
    def fn(thr):
        thr = np.asarray(thr)
        assert thr.dtype == np.int64 and thr.shape == (len(rows), 16)
        assert np.all(thr[:, 1:] >= thr[:, :-1]), "rows of thresholds must be ascending"
        if log is not None:
            log.append(thr.copy())
        return np.stack([np.searchsorted(r, thr[q], side="right") for q, r in enumerate(rows)]).astype(np.int64)
    return fn


def test_pass_bound_values():
    from ganleaks_amd.attack import kth_pass_bound
    assert [kth_pass_bound(s) for s in (0, 15, 16, 287, 288, 65025 * 12288, 2 ** 32 - 1, 2 ** 40)] == [1, 1, 2, 2, 3, 8, 8, 10]
    for s in (0, 1, 15, 16, 287, 288, 65025 * 768, 65025 * 12288, 2 ** 40):
        assert kth_pass_bound(s) == _bound(s) == (math.ceil(math.log(s + 2, 17) - 1e-12) if s > 0 else 1)


@pytest.mark.parametrize("s_max", [0, 1, 15, 16, 17, 271, 272, 287, 288, 4912, 65025 * 768, 65025 * 12288, 2 ** 32 - 1, 2 ** 40])
def test_select_kth_rows_against_sort(s_max):
    from ganleaks_amd.attack import select_kth_rows
    rng = np.random.default_rng(s_max % 1000 + 7)
    nq, n = 23, 57
    rows = []
    for q in range(nq):
        style = q % 5
        if style == 0:
            r = rng.integers(0, s_max + 1, size=n)                                   # spread over the whole range
        elif style == 1:
            r = rng.integers(0, min(s_max, 3) + 1, size=n)                           # heavy ties near 0, S = 0 present
            r[0] = 0
        elif style == 2:
            r = np.full(n, s_max)                                                    # everything at the top
        elif style == 3:
            r = np.repeat(rng.integers(0, s_max + 1, size=n // 3), 3)                # every value three times: the k-th and (k+1)-th tie
        else:
            r = s_max - rng.integers(0, min(s_max, 40) + 1, size=n)                  # dense just below the top
        rows.append(np.sort(r.astype(np.int64)))
    for k in (1, 2, 3, 19, len(rows[3]), n):
        kk = np.minimum(k, [len(r) for r in rows]).astype(np.int64)                  # k = n where the multiset has n elements
        log = []
        S, passes = select_kth_rows(_count_fn(rows, log), kk, nq, s_max)
        assert S.dtype == np.int64 and S.shape == (nq,)
        assert np.array_equal(S, [r[kk[q] - 1] for q, r in enumerate(rows)]), (s_max, k)
        assert 1 <= passes == len(log) <= _bound(s_max), (s_max, k, passes)
    # a scalar k, and k = 1 with S = 0
    S, _ = select_kth_rows(_count_fn(rows), 1, nq, s_max)
    assert np.array_equal(S, [r[0] for r in rows]) and S[1] == 0
    # k beyond the total raises
    with pytest.raises(ValueError):
        select_kth_rows(_count_fn(rows), n + 1, nq, s_max)
    short = np.full(nq, 1, np.int64)
    short[3] = len(rows[3]) + 1
    with pytest.raises(ValueError):
        select_kth_rows(_count_fn(rows), short, nq, s_max)


def test_select_kth_rows_first_pass_and_refusals():
    from ganleaks_amd.attack import select_kth_rows
    rows = [np.sort(np.random.default_rng(3).integers(0, 65025 * 12288, size=100)).astype(np.int64)] * 4
    log = []
    S, passes = select_kth_rows(_count_fn(rows, log), 50, 4, 65025 * 12288)
    assert passes <= 8 and np.all(S == rows[0][49])
    assert np.all(log[0][:, -1] == 65025 * 12288), "the first pass carries s_max: the per-query total"
    assert np.all(log[0][:, 0] >= 0) and len(set(log[0][0].tolist())) == 16
    # k beyond the total is refused after ONE pass where the first pass carries s_max
    log = []
    with pytest.raises(ValueError):
        select_kth_rows(_count_fn(rows, log), 101, 4, 65025 * 12288)
    assert len(log) == 1
    for bad in (0, -1, 1.5, [1, 2, 3], None):
        with pytest.raises(ValueError):
            select_kth_rows(_count_fn(rows), bad, 4, 100)
    with pytest.raises(ValueError):
        select_kth_rows(lambda thr: np.zeros((4, 3), np.int64), 1, 4, 100)
    S, passes = select_kth_rows(_count_fn([]), 1, 0, 100)
    assert S.shape == (0,) and passes == 0


@pytest.mark.parametrize("kind,d", [("u8", 192), ("u8", 12288), ("u8", 270000), ("int", 300), ("int", 1071)])
def test_eps_to_ssd_rows_equals_eps_to_ssd(kind, d):
    from ganleaks_amd.attack import _dist32, eps_to_ssd, eps_to_ssd_rows
    rng = np.random.default_rng(d)
    s_max = 65025 * d
    S = np.concatenate([[0, 1, 2, s_max - 1, s_max], rng.integers(0, s_max + 1, size=27), rng.integers(0, 2000, size=8)])
    exact = _dist32(S, d, kind).astype(np.float32)           # exact float32 distances of some S, and their float32 neighbours
    vals = np.concatenate([exact, np.nextafter(exact, np.float32(-np.inf)), np.nextafter(exact, np.float32(np.inf)),
                           np.asarray([-1.0, -0.0, 0.0, -np.inf, np.inf, 1e-30, 1e30, 3.5, 4.0, float(np.nextafter(np.float32(4.0), np.float32(5.0)))], np.float32),
                           rng.random(6).astype(np.float32) * 4.0]).astype(np.float64)
    vals = vals[: (len(vals) // 16) * 16].reshape(-1, 16)
    got = eps_to_ssd_rows(vals, d, kind)
    assert got.dtype == np.int64 and got.shape == vals.shape
    want = np.stack([eps_to_ssd(row, d, kind) for row in vals])
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert got.min() == -1 and got.max() == s_max
    # a single column, float32 input
    assert np.array_equal(eps_to_ssd_rows(vals[:, :1].astype(np.float32), d, kind), want[:, :1])


def test_eps_to_ssd_rows_refusals():
    from ganleaks_amd.attack import eps_to_ssd_rows
    for bad in ([1.0, 2.0], np.zeros((3, 17)), np.zeros((3, 0)), [[np.nan]], np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            eps_to_ssd_rows(bad, 768)
    with pytest.raises(ValueError):
        eps_to_ssd_rows([[1.0]], 768, "f32")
    with pytest.raises(ValueError):
        eps_to_ssd_rows([[1.0]], 0)
    assert eps_to_ssd_rows(np.zeros((0, 3)), 768).shape == (0, 3)


def test_density_ratio_loss_and_its_clamp():
    from ganleaks_amd.attack import density_ratio_loss
    a = np.asarray([0, 1, 2, 100, 65025 * 12288, 0], np.int64)
    b = np.asarray([0, 0, 1, 400, 1, 65025 * 12288], np.int64)
    got = density_ratio_loss(a, b)
    assert got.dtype == np.float64 and np.all(np.isfinite(got))
    want = [0.0, 0.0, 0.5 * math.log(2.0), 0.5 * (math.log(100.0) - math.log(400.0)), 0.5 * math.log(65025.0 * 12288), -0.5 * math.log(65025.0 * 12288)]
    assert np.array_equal(got, np.asarray(want, np.float64))
    # exact duplicates (S = 0) score as the smallest non-zero S does, and the loss is the log ratio of the radii
    assert np.array_equal(density_ratio_loss([0], [7]), density_ratio_loss([1], [7]))
    assert abs(got[3] - math.log(math.sqrt(100.0) / math.sqrt(400.0))) < 1e-15
    # monotone: closer under the bank, or farther under the reference set, is more member-like (smaller)
    assert density_ratio_loss([10], [50]) < density_ratio_loss([11], [50]) and density_ratio_loss([10], [51]) < density_ratio_loss([10], [50])


NO_GPU_CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
import numpy as np
import ganleaks_amd as gl
from ganleaks_amd import _lib, shard
def no_context(*a, **k):
    raise AssertionError("a Context was asked for")
_lib.Context.get = staticmethod(no_context)
_lib.Context.__init__ = no_context
q = np.zeros((4, 3, 8, 8), np.uint8)
bank = np.zeros((64, 3, 8, 8), np.uint8)
def raises(exc, fn, *a, **k):
    try:
        fn(*a, **k)
    except exc:
        return
    raise SystemExit("no %%s from %%s%%r" %% (exc.__name__, fn.__name__, (a[2:], k)))
for bad in (0, -3, 1.5, "3", [1, 0], [[1, 2]], list(range(1, 18)), [], True, None):
    raises(ValueError, gl.kth_distances, q, bank, bad)
    raises(ValueError, shard.kth_distances_on_devices, q, bank=bank, k=bad, devices=[0])
raises(ValueError, gl.kth_distances, q, bank, 1, distance="cosine")
raises(NotImplementedError, gl.kth_distances, q, bank, 1, distance="l2-lpips")
for bad in (1.0, [1.0, 2.0], np.zeros((4, 17)), np.zeros((4, 0)), np.zeros((3, 2)), np.full((4, 2), np.nan)):
    raises(ValueError, gl.ball_counts_rows, q, bank, bad)
raises(ValueError, gl.ball_counts_rows, q, bank, np.zeros((4, 2)), distance="cosine")
raises(NotImplementedError, gl.ball_counts_rows, q, bank, np.zeros((4, 2)), distance="l2-lpips")
print("refused")
'''


def test_argument_errors_come_before_any_context():
    r = subprocess.run([sys.executable, "-c", NO_GPU_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("refused"), r.stdout + r.stderr


def test_density_refusals(tmp_path, monkeypatch):
    from ganleaks_amd.attack_models import density
    monkeypatch.chdir(tmp_path)
    os.makedirs(tmp_path / "syn")
    base = ["--syn_data_path", str(tmp_path / "syn"), "--pos_data_dir", str(tmp_path / "nowhere"), "--neg_data_dir", str(tmp_path / "nowhere")]
    # the folders are empty or missing: refused before anything is read
    for extra, needle in ((["--distance", "l2-lpips"], "l2-lpips is not built"), (["--distance", "cosine"], "--distance must be l2"),
                          (["--K", "0"], "--K must be"), (["--K", "-4"], "--K must be"), (["--K_ref", "3"], "--K_ref needs --ref_data_dir"),
                          (["--K_ref", "0", "--ref_data_dir", str(tmp_path / "syn")], "--K_ref must be")):
        with pytest.raises(SystemExit) as e:
            density.main(density.parse_arguments(base + extra))
        assert needle in str(e.value), (extra, str(e.value))
    args = density.parse_arguments(base)
    args.K = 2.5                             # as a YAML overlay could set it
    with pytest.raises(SystemExit):
        density.main(args)
    assert not (tmp_path / "density_attack").exists()
    d = density.parse_arguments(base)
    assert d.K is None and d.K_ref is None and d.ref_data_dir is None and d.distance == "l2" and d.BATCH_SIZE == 30
    assert density.density_request(density.parse_arguments(base + ["--K", "316"])) == (316, None)


def test_entry_points_are_declared_bound_and_exported():
    import ganleaks_amd
    from ganleaks_amd import _lib, shard
    code = open(os.path.join(ROOT, "include", "ganleaks.h")).read()
    for name in ("gl_l2_count_rows_i8", "gl_l2_count_rows_i8_wide"):
        assert re.search(r"\bint %s\(gl_ctx \*ctx," % name, code), name
        assert re.search(r'"%s": \(_i, \[' % name, open(_lib.__file__).read()), name
    assert re.search(r"#define\s+GL_ABI_VERSION\s+1\b", code)
    for name in ("ball_counts_rows", "count_balls_rows", "eps_to_ssd_rows", "kth_distances", "select_kth_rows"):
        assert callable(getattr(ganleaks_amd, name)), name
    assert callable(shard.DeviceGroup.kth_distances) and callable(shard.kth_distances_on_devices)


def test_rows_kernels_keep_their_k_loops_free_of_scratch():
    """the four instantiations with per-query thresholds, by the assembly (no GPU needed): no spill inside the K loop, and the hand-placed
    fragment reads of the 256 x 256 tile stay untouched while in flight"""
    kernels = ["l2_count_rows_i8_kernelILb0EiE", "l2_count_rows_i8_kernelILb1EiE", "l2_count_rows_i8_kernelILb1ElE", "l2_count_rows_i8_256p_kernel"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_loop_spills.py"), "--kernels", ",".join("gl_count_rows.hip:" + k for k in kernels),
                        "--pipelined", "gl_count_rows.hip:l2_count_rows_i8_256p_kernel"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("0 scratch instructions inside the K loop") == 4 and "not found" not in r.stdout, r.stdout
    assert r.stdout.count(", 0 instructions touch a fragment register still in flight") == 1, r.stdout
