"""bench.py's rank launcher on a machine without GPUs: it must refuse (non-zero exit, message) before touching a device."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_gpus_n_refuses_without_enough_gpus():
    import torch
    if torch.cuda.device_count() >= 2:
        return
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--gpus 2 but only" in r.stderr and not r.stdout.strip()


def test_bench_has_full_and_dump_outputs_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout, r.stderr[-2000:]


def test_dump_outputs_writes_float32_and_a_fixed_sample_over_the_cap(tmp_path, monkeypatch):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    mols = [(torch.tensor([3, 1]), torch.tensor([[0, 2], [2, 0]])), (torch.tensor([4, 4, 0]), torch.zeros(3, 3, dtype=torch.long))]
    arrays = dict(bench.pack_molecules(mols, 4), loss=np.array([0.25]))
    assert arrays["atom_types"].tolist() == [[3, 1, -1, -1], [4, 4, 0, -1]] and arrays["n_atoms"].tolist() == [2, 3]
    assert arrays["edge_types"][0, :2, :2].tolist() == [[0, 2], [2, 0]] and (arrays["edge_types"][0, 2:] == -1).all()
    bench.dump_outputs(str(tmp_path / "all"), dict(arrays, tokens=np.arange(6).reshape(2, 3)))
    got = {k: np.load(str(tmp_path / "all" / (k + ".npy"))) for k in ("atom_types", "edge_types", "n_atoms", "loss", "tokens")}
    assert {k: v.dtype for k, v in got.items()} == {"atom_types": np.float32, "edge_types": np.float32, "n_atoms": np.float32,
                                                    "loss": np.float64, "tokens": np.float32}
    np.testing.assert_array_equal(got["edge_types"], arrays["edge_types"])
    # over the cap every array keeps the same seeded share of its rows, the same from call to call
    big = {"x": np.arange(4000, dtype=np.float32).reshape(1000, 4)}
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4000)
    for name in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / name), big)
    s1, s2 = np.load(str(tmp_path / "s1" / "x.npy")), np.load(str(tmp_path / "s2" / "x.npy"))
    assert s1.nbytes <= 4000 and s1.shape == (250, 4) and np.array_equal(s1, s2) and (np.diff(s1[:, 0]) > 0).all()
