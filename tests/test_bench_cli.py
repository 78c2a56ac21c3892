"""GPU: bench.py as the driver runs it.  A plain run times exactly --steps steps, prints one JSON line without the --full
measurements, and --dump-outputs writes the intervals the last timed step calibrated -- the same intervals a calibration of the
same seeded network and images gives in this process."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_steps_and_dumps_what_the_last_step_computed(tmp_path):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "deit_tiny_patch16_224", "--config", "BasePTQ",
           "--calib", "4", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "layers/s" and d["higher_is_better"] is True
    assert d["dtype"] == "int8" and d["metric"].startswith("calibration throughput") and d["ms_per_step"] > 0
    for k in ("roofline", "cpu_baseline", "steady_state_recalibration_s", "fresh_network_eager_capture_s", "quant_forward", "top1"):
        assert d[k] is None, k          # --full only

    got = {f[:-len(".npy")]: np.load(out / f) for f in os.listdir(out)}
    modules = {k.rsplit(".", 1)[0] for k in got}
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - len(modules)) < 1e-6 * len(modules)     # value = modules x steps / time
    assert all(v.dtype == np.float32 for v in got.values())

    from ptq4vit_amd.configs import BasePTQ
    from ptq4vit_amd.utils import models, net_wrap
    from ptq4vit_amd.utils.intervals import module_intervals
    from ptq4vit_amd.utils.quant_calib import HessianQuantCalibrator
    net = models.get_net("deit_tiny_patch16_224", seed=0, device="cuda")
    images = torch.randn(4, 3, 224, 224, generator=torch.Generator(device="cpu").manual_seed(0)).cuda()

    class Loader:           # bench.py's SyntheticLoader: one batch of all images
        batch_size = 4

        def __iter__(self):
            yield images, torch.zeros(4, dtype=torch.long)

    with contextlib.redirect_stdout(io.StringIO()):
        wrapped = net_wrap.wrap_modules_in_net(net, BasePTQ)
        HessianQuantCalibrator(net, wrapped, Loader(), sequential=False, batch_size=4).batching_quant_calib()
    torch.cuda.synchronize()
    want = {f"{n}.{a}": t.numpy() for n, m in wrapped.items() for a, t in module_intervals(m).items()}
    assert set(got) == set(want)
    for k, v in want.items():
        assert np.array_equal(got[k], v), f"{k}: dumped {got[k].ravel()[:3]} vs in-process {v.ravel()[:3]}"
