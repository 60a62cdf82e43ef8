"""bench.py's options on CPU: a plain run is the default and `--full` opts into the extra measurements; `--dump-outputs`
writes the frame as float32 .npy files, bit for bit, cut to a fixed seeded pixel sample when it would exceed the budget."""
import os

import numpy as np
import pytest


@pytest.fixture
def bench(monkeypatch):
    # bench.py sets an HSA variable for itself at import: this process's environment is restored afterwards
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    import bench
    return bench


def _frame(h, w, seed=3):
    rng = np.random.default_rng(seed)
    rgb = rng.random((h, w, 3), dtype=np.float32)
    rgb[0, 0, 1] = np.nan
    rgba = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32)
    return rgb, rgba


def test_plain_run_is_the_default(bench):
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_zero_steps_is_an_error(bench):
    with pytest.raises(SystemExit) as e:
        bench.main(["--steps", "0"])
    assert "--steps" in str(e.value)


def test_dump_outputs_writes_the_frame_bit_for_bit(bench, tmp_path):
    rgb, rgba = _frame(5, 7)
    names = bench.dump_outputs(str(tmp_path), rgb, rgba[..., None].view(np.int32))  # (the torch path hands over int32 words)
    assert names == ["rgb", "rgba8"]
    got, got8 = np.load(tmp_path / "rgb.npy"), np.load(tmp_path / "rgba8.npy")
    assert got.dtype == np.float32 and got8.dtype == np.float32
    assert got.shape == (5, 7, 3) and got.tobytes() == rgb.tobytes()
    assert got8.shape == (5, 7, 4)
    for c, shift in enumerate((0, 8, 16, 24)):  # 0xAABBGGRR -> R, G, B, A
        assert np.array_equal(got8[..., c], ((rgba >> shift) & 0xff).astype(np.float32))


def test_dump_outputs_samples_a_large_frame_within_the_budget(bench, tmp_path):
    rgb, rgba = _frame(40, 50)
    budget = 28 * 1000  # bytes, for 2000 pixels of 28 (rgb + rgba8) and 8 more per sampled pixel's index
    for d in ("a", "b"):
        names = bench.dump_outputs(str(tmp_path / d), rgb, rgba, budget=budget)
        assert names == ["pixel_index", "rgb", "rgba8"]
    arrays = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in names}
    assert sum(a.nbytes for a in arrays.values()) <= budget
    for n in names:  # the same sample every time
        assert np.load(tmp_path / "b" / f"{n}.npy").tobytes() == arrays[n].tobytes()
    idx = arrays["pixel_index"]
    assert idx.dtype == np.float64 and len(idx) == budget // 36 and np.all(np.diff(idx) > 0)
    flat = idx.astype(np.int64)
    assert arrays["rgb"].tobytes() == rgb.reshape(-1, 3)[flat].tobytes()
    assert np.array_equal(arrays["rgba8"][:, 0], (rgba.reshape(-1)[flat] & 0xff).astype(np.float32))
