"""CPU: the float_path keyword of the top-K / ball-count entry points, the row reader of the attack drivers (bank_io.load_rows) and the
golden of the off-lattice search (tests/golden/knn_float_rows.npz) against the CPU chain.  No GPU is touched."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import float_rows_common as common

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("gl_l2_topk_f32", "gl_l2_count_f32")


def test_float_path_is_in_the_signatures():
    import importlib
    from ganleaks_amd import shard
    attack = importlib.import_module("ganleaks_amd.attack")
    for fn in (attack.ball_counts, attack.nearest_neighbours, shard.DeviceGroup.ball_counts, shard.DeviceGroup.nearest_neighbours,
               shard.ball_counts_on_devices, shard.nearest_neighbours_on_devices):
        assert inspect.signature(fn).parameters["float_path"].default is None, fn
    assert "float_path" not in inspect.signature(attack.pair_distances).parameters


def test_keyword_is_checked_before_any_context():
    """a machine without a GPU cannot create a Context: these raise what the keyword check raises"""
    import importlib
    from ganleaks_amd import shard
    attack = importlib.import_module("ganleaks_amd.attack")
    q, b = np.full((2, 5), 0.3, np.float32), np.full((8, 5), 0.7, np.float32)
    for bad in ("bogus", "EXACT", "", 1, True):
        with pytest.raises(ValueError, match="float_path"):
            attack.ball_counts(q, b, 0.5, batch_size=4, float_path=bad)
        with pytest.raises(ValueError, match="float_path"):
            attack.nearest_neighbours(q, b, 2, distance="l2", batch_size=4, float_path=bad)
        with pytest.raises(ValueError, match="float_path"):
            shard.ball_counts_on_devices(q, bank=b, eps=0.5, batch_size=4, devices=[0, 0], float_path=bad)
        with pytest.raises(ValueError, match="float_path"):
            shard.nearest_neighbours_on_devices(q, bank=b, k=2, batch_size=4, devices=[0, 0], distance="l2", float_path=bad)
    for call in (lambda: attack.ball_counts(q, b, 0.5, batch_size=4, float_path="mfma"),
                 lambda: attack.nearest_neighbours(q, b, 2, distance="l2", batch_size=4, float_path="mfma"),
                 lambda: shard.ball_counts_on_devices(q, bank=b, eps=0.5, batch_size=4, devices=[0, 0], float_path="mfma")):
        with pytest.raises(NotImplementedError, match="mfma"):
            call()


def test_exports_are_declared_and_bound():
    from ganleaks_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    for name in NEW_EXPORTS:
        assert name in _lib.SIGNATURES and ("int %s(gl_ctx *ctx" % name) in header
    assert "fbb.py:73-88" in header[header.index("gl_l2_topk_f32"):] and "utils.py:163" in header[header.index("gl_l2_count_f32"):]


def test_host_rows_kind():
    from ganleaks_amd.attack import host_rows_kind
    codes = np.arange(256, dtype=np.uint8).reshape(4, 64)
    assert host_rows_kind(codes) == "u8" and host_rows_kind(common.decode_u8(codes)) == "u8"
    assert host_rows_kind(codes.astype(np.float32)) == "int" and host_rows_kind((codes > 100).astype(np.float64)) == "int"
    off = common.decode_u8(codes)
    off[3, 5] += np.float32(1e-4)
    assert host_rows_kind(off) == "f32" and host_rows_kind(codes.astype(np.float32) + np.float32(0.5)) == "f32"
    with pytest.raises(TypeError):
        host_rows_kind(codes.astype(np.int32))


def test_load_rows(tmp_path):
    from ganleaks_amd.bank_io import concat_rows, load_rows
    rng = np.random.default_rng(3)
    x = rng.random((5, 8, 8, 3), dtype=np.float32)                      # NHWC in [0, 1), as gan_models/vaegan/sample.py writes it
    np.savez_compressed(tmp_path / "generated.npz", noise=np.zeros((5, 4), np.float32), img_r01=x)
    rows = load_rows(str(tmp_path / "generated.npz"), 8)
    assert rows.dtype == np.float32 and rows.shape == (5, 3, 8, 8) and rows.flags["C_CONTIGUOUS"]
    assert np.array_equal(rows, (np.float32(2.0) * x - np.float32(1.0)).transpose(0, 3, 1, 2))
    assert rows[2, 1, 4, 6] == np.float32(np.float32(2.0) * x[2, 4, 6, 1] - np.float32(1.0))
    with pytest.raises(ValueError, match="not resized"):
        load_rows(str(tmp_path / "generated.npz"), 16)
    np.savez(tmp_path / "other.npz", fake=x)
    with pytest.raises(ValueError, match="img_r01"):
        load_rows(str(tmp_path / "other.npz"), 8)
    table = rng.normal(0.0, 1.5, (7, 37))
    np.save(tmp_path / "synthetic.npy", table)
    got = load_rows(str(tmp_path / "synthetic.npy"), 64)
    assert got.dtype == np.float32 and np.array_equal(got, table.astype(np.float32))
    np.save(tmp_path / "cube.npy", np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError):
        load_rows(str(tmp_path / "cube.npy"), 64)
    with pytest.raises(ValueError):
        load_rows(str(tmp_path / "rows.txt"), 64)
    # a PNG folder: 8-bit codes, as load_png_bank reads them
    import PIL.Image
    codes = rng.integers(0, 256, (3, 3, 8, 8), dtype=np.uint8)
    os.makedirs(tmp_path / "png")
    for i, im in enumerate(codes):
        PIL.Image.fromarray(im.transpose(1, 2, 0)).save(tmp_path / "png" / ("image_%d.png" % i))
    from_dir = load_rows(str(tmp_path / "png"), 8)
    assert from_dir.dtype == np.uint8 and np.array_equal(from_dir, codes)
    # codes next to floats are decoded before they are joined
    both = concat_rows(from_dir, rows)
    assert both.dtype == np.float32 and np.array_equal(both[:3], common.decode_u8(codes)) and np.array_equal(both[3:], rows)
    assert concat_rows(from_dir, from_dir).dtype == np.uint8


def test_table_under_lpips_is_refused(tmp_path, monkeypatch):
    from ganleaks_amd.attack_models import knn, mc
    np.save(tmp_path / "t.npy", np.zeros((40, 5), np.float32))
    monkeypatch.chdir(tmp_path)
    t = str(tmp_path / "t.npy")
    base = ["--syn_data_path", t, "--pos_data_dir", t, "--neg_data_dir", t, "--BATCH_SIZE", "10", "--distance", "l2-lpips"]
    with pytest.raises(SystemExit, match="l2-lpips needs images"):
        knn.main(knn.parse_arguments(base))
    with pytest.raises(SystemExit, match="l2-lpips needs images"):
        mc.main(mc.parse_arguments(base + ["--eps", "0.5"]))


def test_golden_rederives(synth, golden_dir):
    """the stored reference order is the chain's stable order on the rows re-derived from the stored seeds, with the margin the generator
    asserted: the GPU test may compare every slot of every query"""
    g = np.load(os.path.join(golden_dir, "knn_float_rows.npz"))
    keep = int(g["keep"])
    names = [n for n, _, _ in common.golden_cases()]
    assert int(g["n_cases"]) == len(names) == 4 and keep == common.KEEP
    for c, (name, kind, params) in enumerate(common.golden_cases()):
        assert str(g["name%d" % c]) == name and str(g["kind%d" % c]) == kind and g["params%d" % c].tolist() == list(params)
        bank, queries, bs = common.derive(synth, kind, g["params%d" % c])
        assert bank.dtype == np.float32 and queries.dtype == np.float32
        n_eff = (len(bank) // bs) * bs
        M = common.chain_matrix(queries, bank[:n_eff])
        order = np.argsort(M, axis=1, kind="stable")[:, :keep + 1]
        chain = np.take_along_axis(M, order, axis=1).astype(np.float64)
        assert np.array_equal(g["idx%d" % c], order[:, :keep]), name
        err = float(g["err%d" % c])
        assert np.max(np.abs(g["dist%d" % c].astype(np.float64) - chain[:, :keep])) <= err, name
        assert np.min(np.diff(chain, axis=1)) > 4.0 * err, name


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_no_spills_in_the_pair_kernels(tmp_path):
    """the three epilogues share one K loop (pair_tile_f32); none of the instantiations may touch scratch, and none may carry the
    accumulators through accumulator-register copies (a counting epilogue that read the K loop's registers directly made the compiler move
    221 of them per K slice: invisible to every parity test, a third of the loop's VALU work)"""
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    src = os.path.join(ROOT, "gan-leaks_amd", "csrc", "gl_l2f32.hip")
    out = str(tmp_path / "gl_l2f32.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only", "-S", src, "-o", out], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    for epi in (0, 1, 2):
        m = re.search(r"^(_Z\S*l2_pairs_f32_kernelILi%dE\S*):" % epi, asm, re.M)
        assert m, epi
        body = asm[m.end():asm.index(".amdhsa_kernel " + m.group(1))]
        assert "v_fma_f32" in body or "v_fmac_f32" in body or "v_pk_fma_f32" in body
        assert body.count("scratch_") == 0, (epi, body.count("scratch_"))
        assert body.count("v_accvgpr") <= 64, (epi, body.count("v_accvgpr"))
