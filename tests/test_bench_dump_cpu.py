"""bench.py --dump-outputs without a GPU: dump_outputs on record sets unpacked by the pipeline's own RecordLayout from random bytes --
float32 files of fixed shapes, the defined entries unchanged, zero past every count, the match rows paired with the frame in front,
and above the size limit a fixed, seeded sample of frames."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from orb_slam2_aruco_amd.pipeline import RecordLayout, RecordLayoutC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records(B, cap, mcap, seed):
    """A record set with random contents (the orbfe_record_layout order of include/orbfe.h), counts in range, and its matches."""
    c = RecordLayoutC(frames=B, capacity=cap, marker_capacity=mcap, halo=1)
    off = 0
    for name, size in (("off_kps", (B + 1) * cap * 28), ("off_desc", (B + 1) * cap * 32), ("off_n", (B + 1) * 4),
                       ("off_markers", B * mcap * 36), ("off_nmarkers", B * 4), ("off_poses", B * mcap * 56)):
        setattr(c, name, off)
        off += size
    c.nbytes = off
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, off, dtype=np.uint8)
    rec = RecordLayout(c).unpack(buf)
    rec["n"][:] = rng.integers(0, cap + 1, B)
    rec["halo_n"][:] = rng.integers(0, cap + 1, 1)
    rec["nmk"][:] = rng.integers(0, mcap + 3, B)                  # the count may exceed the stored markers
    for k in ("x", "y", "size", "angle", "response"):            # finite floats (random bytes make NaNs)
        rec["kps"][k] = rng.uniform(0, 100, rec["kps"].shape)
        rec["halo_kps"][k] = rng.uniform(0, 100, rec["halo_kps"].shape)
    rec["kps"]["octave"] = rng.integers(0, 8, rec["kps"].shape)
    rec["halo_kps"]["octave"] = rng.integers(0, 8, rec["halo_kps"].shape)
    rec["markers"]["id"] = rng.integers(0, 1024, rec["markers"].shape)
    rec["markers"]["corners"] = rng.uniform(0, 640, rec["markers"]["corners"].shape)
    for k in ("rvec", "tvec", "rvec2", "tvec2", "err"):
        rec["poses"][k] = rng.normal(size=rec["poses"][k].shape)
    matches = {k: rng.integers(-1, cap, (B, cap)).astype(np.int32) for k in ("best_idx", "best_dist", "second_dist", "matches12")}
    matches["nmatches"] = rng.integers(0, cap, B).astype(np.int32)
    return rec, matches


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_holds_the_defined_records_as_float32(tmp_path):
    B, cap, mcap = 6, 40, 3
    rec, matches = _records(B, cap, mcap, 1)
    sidx = (np.arange(B) + 2) % B
    names = bench.dump_outputs(str(tmp_path), rec, matches, sidx, 5)
    d = _load(tmp_path)
    assert sorted(d) == names and all(a.dtype == np.float32 for a in d.values())
    assert np.array_equal(d["frame_index"], sidx) and d["halo_frame_index"].tolist() == [5]
    assert d["keypoints"].shape == (B, cap, 7) and d["descriptors"].shape == (B, cap, 32) and d["markers"].shape == (B, mcap, 9)
    assert d["poses"].shape == (B, mcap, 14) and d["knn2_best_idx"].shape == (B, cap)
    n, n1 = rec["n"], np.concatenate([rec["halo_n"], rec["n"][:-1]])
    for f in range(B):
        k = int(n[f])
        assert d["n_keypoints"][f] == k
        assert np.array_equal(d["keypoints"][f, :k, 0], rec["kps"]["x"][f, :k]) and np.array_equal(d["keypoints"][f, :k, 5], rec["kps"]["octave"][f, :k])
        assert np.array_equal(d["descriptors"][f, :k], rec["desc"][f, :k]) and not d["descriptors"][f, k:].any() and not d["keypoints"][f, k:].any()
        for name, key in (("knn2_best_idx", "best_idx"), ("knn2_second_dist", "second_dist"), ("init_matches12", "matches12")):
            assert np.array_equal(d[name][f, :n1[f]], matches[key][f, :n1[f]]) and not d[name][f, n1[f]:].any(), (name, f)
        m = min(int(rec["nmk"][f]), mcap)
        assert d["n_markers"][f] == rec["nmk"][f] and np.array_equal(d["markers"][f, :m, 0], rec["markers"]["id"][f, :m])
        assert np.array_equal(d["markers"][f, :m, 1:].reshape(m, 4, 2), rec["markers"]["corners"][f, :m]) and not d["markers"][f, m:].any()
        assert np.array_equal(d["poses"][f, :m, 3:6], rec["poses"]["tvec"][f, :m]) and not d["poses"][f, m:].any()
    h = int(rec["halo_n"][0])
    assert np.array_equal(d["halo_descriptors"][0, :h], rec["halo_desc"][0, :h]) and not d["halo_descriptors"][0, h:].any()
    assert np.array_equal(d["init_n_matches"], matches["nmatches"])


def test_dump_above_the_limit_is_a_fixed_sample(tmp_path, monkeypatch):
    B, cap, mcap = 40, 64, 4
    rec, matches = _records(B, cap, mcap, 2)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 400_000)
    bench.dump_outputs(str(tmp_path / "a"), rec, matches, np.arange(B), B - 1)
    rec2, matches2 = _records(B, cap, mcap, 3)                    # other contents, same shapes: the same frames
    bench.dump_outputs(str(tmp_path / "b"), rec2, matches2, np.arange(B), B - 1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    fids = a["frame_index"].astype(int)
    assert 1 < len(fids) < B and np.array_equal(fids, b["frame_index"]) and np.all(np.diff(fids) > 0)
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in a) <= 400_000
    for i, f in enumerate(fids):
        k = int(rec["n"][f])
        assert np.array_equal(a["descriptors"][i, :k], rec["desc"][f, :k])
        n1 = int(rec["n"][f - 1]) if f else int(rec["halo_n"][0])
        assert np.array_equal(a["knn2_best_dist"][i, :n1], matches["best_dist"][f, :n1])


def test_dump_without_the_aruco_leg(tmp_path):
    rec, matches = _records(4, 16, 2, 4)
    names = bench.dump_outputs(str(tmp_path), rec, matches, np.arange(4), 3, use_aruco=False)
    assert "markers" not in names and "poses" not in names and "descriptors" in names


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--latency", "--dump-outputs", "x"]])
def test_bench_refuses_bad_arguments(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--launch-check", *argv], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "error" in r.stderr
