"""bench.py end to end on a small grid: a plain run prints the headline fields and nothing else, --full adds the rest; the x both
runs dump comes out of the same timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
            "config"}


def _bench(*extra, dump):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--grid", "200",
                        "--dump-outputs", str(dump)] + list(extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(tmp_path):
    plain = _bench(dump=tmp_path / "plain")
    assert set(plain) == HEADLINE
    assert plain["value"] == plain["ms_per_step"] > 0.0 and plain["unit"] == "ms" and plain["higher_is_better"] is False
    assert plain["dtype"] == "f64" and (plain["steps"], plain["warmup"]) == (2, 1)

    full = _bench("--full", "--no-extras", "--no-cpu-baseline", dump=tmp_path / "full")
    assert HEADLINE < set(full)
    assert {"phases_ms", "factor", "roofline", "roofline_factor", "total_ifs_ms"} <= set(full)
    assert full["relative_error"] < 1e-12

    x_plain, x_full = np.load(tmp_path / "plain" / "x.npy"), np.load(tmp_path / "full" / "x.npy")
    assert x_plain.shape == x_full.shape == (200 * 200,)
    assert np.allclose(x_plain, x_full, rtol=1e-12, atol=0.0)
