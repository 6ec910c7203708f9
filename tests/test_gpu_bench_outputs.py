"""bench.py --dump-outputs: what the last timed step left, for comparing two builds.

One small leg of bench.run_leg (the bench shape 64 x 64, 24 envs, T = 6) per schedule,
ending inside an episode (the fused schedule has then selected for the next row) and at an
episode's end (no selection follows).  The files are
float32 / float64, hold the rows of the step they name (the batch's own invariants: the
one-hot of the actions, prev_assigns == the actions taken, obs one-hot block, beta == obs
block 1), and a second run with the same arguments writes the same bytes.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

DEV = torch.device("cuda", 0)
E, N, M, T = 24, 64, 64, 6


def _dump(path, steps, warmup, fused):
    a = bench.parse(["--n", str(N), "--m", str(M), "--envs", str(E), "--T", str(T), "--fused-rollout", str(fused)])
    res = bench.run_leg(a, DEV, 1, E, steps, warmup, dump_dir=str(path))
    assert res["mode"] == ("episode" if fused else None)
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("steps,warmup,next_selected", [(5, 4, True), (9, 3, False)])
def test_dump_outputs_rows_and_repeatability(tmp_path, steps, warmup, next_selected, fused):
    d = _dump(tmp_path / "a", steps, warmup, fused)
    # the fused schedules select for row t + 1 inside the step; the split schedule's last step does not
    expect = {"actions", "actions_onehot", "rewards", "terminated", "obs", "avail_actions", "prev_assigns", "beta",
              "hidden_states", "returns", "env_index"} | ({"next_actions"} if next_selected and fused else set())
    assert set(d) == expect
    for k, v in d.items():
        assert v.dtype == (np.float64 if k in ("returns", "env_index") else np.float32), k
        assert np.isfinite(v).all(), k
    assert sum(v.nbytes for v in d.values()) <= 64 << 20
    assert np.array_equal(d["env_index"], np.arange(E))  # every env fits the budget here
    act = d["actions"][:, :, 0].astype(np.int64)
    assert ((act >= 0) & (act < M)).all()
    onehot = np.eye(M, dtype=np.float32)[act]
    assert np.array_equal(d["actions_onehot"], onehot)
    assert np.array_equal(d["prev_assigns"], act.astype(np.float32))
    assert np.array_equal(d["obs"][:, :, :M], onehot)
    assert np.array_equal(d["beta"], d["obs"][:, :, M:2 * M])
    assert d["avail_actions"].all()
    last = (steps + warmup) % T == 0
    assert (d["terminated"] == float(last)).all()
    assert d["returns"].shape == (E,) and d["hidden_states"].shape == (E, N * 64)
    assert np.abs(d["hidden_states"]).max() > 0 and np.abs(d["rewards"]).max() > 0
    if "next_actions" in d:
        assert ((d["next_actions"] >= 0) & (d["next_actions"] < M)).all()
    d2 = _dump(tmp_path / "b", steps, warmup, fused)
    for k, v in d.items():
        assert np.array_equal(v, d2[k]), k
