"""GPU: a pool knows how many hardware queues its process asked for, says so when its workers have to share them, and
computes the same rows either way.  Two fresh processes that both find GPU_MAX_HW_QUEUES=4, one of them with
RSI_HOT_HW_QUEUES=keep: the scale-0.01 genome of the flagship configuration once through a pool of 8 workers.  No timing."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKERS = 8

CHILD = r"""
import hashlib, os, sys
sys.path.insert(0, sys.argv[1])
workers = int(sys.argv[2])
import torch
from rsicnv_amd import api, synth
lib = api.load_library()
dev = torch.device("cuda", 0)
data = []
for c in range(24):
    p = synth.config_plan(4, chrom=c, scale=0.01)
    d_fa = torch.empty(p["n"] + 64, dtype=torch.uint8, device=dev)
    d_rd = torch.empty(p["n"] + 16, dtype=torch.int32, device=dev)
    synth.generate_device(lib, p, d_fa.data_ptr(), d_rd.data_ptr())
    data.append((d_rd, d_fa, p["n"]))
torch.cuda.synchronize()
pool = api.RsiPool(0, workers)
res = pool.run(api.make_params(**synth.config_flags(4)), [(a.data_ptr(), b.data_ptr(), n) for a, b, n in data])
h = hashlib.sha256()
rows = 0
for c, r in enumerate(res):
    for row in r.format_rows(f"chr{c + 1}"):
        h.update(row.encode()); h.update(b"\n")
        rows += 1
    h.update(repr((c, float(r.stats["RDmedian"]), float(r.stats["RDsd"]))).encode())
print(repr((pool.hw_queues, os.environ.get("GPU_MAX_HW_QUEUES"), rows, h.hexdigest())))
pool.close()
"""


def child(keep):
    env = {k: v for k, v in os.environ.items() if k != "RSI_HOT_HW_QUEUES"}
    env["GPU_MAX_HW_QUEUES"] = "4"
    if keep:
        env["RSI_HOT_HW_QUEUES"] = "keep"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(WORKERS)], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-800:]
    return eval(r.stdout.strip().splitlines()[-1]), r.stderr


@pytest.mark.gpu
def test_pool_reports_its_queues_and_rows_do_not_depend_on_them():
    with ThreadPoolExecutor(max_workers=2) as ex:
        (raised, raised_err), (kept, kept_err) = ex.map(child, (False, True))
    print("default:", raised, "keep:", kept)
    assert raised[0] == 32 and raised[1] == "32"
    assert kept[0] == 4 and kept[1] == "4"
    assert raised[2] > 0 and raised[2:] == kept[2:], "the rows of the genome depend on the number of hardware queues"
    # 8 workers > 4 - 2 queues: said once, naming the variable and the function that sets it; 8 <= 32 - 2: nothing to say
    warning = [l for l in kept_err.splitlines() if l.startswith("rsi_pool_create:")]
    assert len(warning) == 1 and "GPU_MAX_HW_QUEUES" in warning[0] and "rsi_hot_process_setup" in warning[0], kept_err[-800:]
    assert "rsi_pool_create:" not in raised_err, raised_err[-800:]
