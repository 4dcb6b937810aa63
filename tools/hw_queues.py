"""The hardware queues a bench.py run started from THIS environment asks the HIP runtime for: what GPU_MAX_HW_QUEUES holds after
`import rsicnv_amd.api` has applied the library's policy (rsi_hot_process_setup, include/rsi_hot.h).  No GPU is touched.  The
tools that print a bench line print this figure beside it: three rounds of profiles were recorded on 4 queues unnoticed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
found = os.environ.get("GPU_MAX_HW_QUEUES", "unset")
from rsicnv_amd import api  # noqa: E402

print(f"{api.HW_QUEUES or 'runtime default (4)'} (found {found}, RSI_HOT_HW_QUEUES {os.environ.get('RSI_HOT_HW_QUEUES', 'unset')})")
