"""CPU: the hardware-queue policy (rsi_hot_process_setup, include/rsi_hot.h) from every starting environment, once as
`import rsicnv_amd.api` applies it (api._process_setup) and once as the native function does, called through ctypes in a
process that never imports the package.  Every child is a fresh process; no HIP call is made anywhere here."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rsicnv_amd", "librsi_hot.so")

STARTS = [None, "4", "2", "16", "32", "64", "junk"]   # GPU_MAX_HW_QUEUES as the process finds it (None: unset)
USERS = [None, "keep", "8", "2", "99"]                # RSI_HOT_HW_QUEUES
# a few starts beyond the issue's list, for the rule "one to nine decimal digits and nothing else": (start, what it must become)
ODD_STARTS = [("", "32"), ("0", "32"), ("+64", "32"), (" 64", "32"), ("064", "064"), ("1234567890", "32")]


def expected(start, user):
    """GPU_MAX_HW_QUEUES afterwards (None: still unset), written out from the policy's text, not from the code under test."""
    if user == "keep":
        return start
    if user is not None:
        return {"8": "8", "2": "4", "99": "32"}[user]
    return {None: "32", "4": "32", "2": "32", "16": "32", "32": "32", "64": "64", "junk": "32"}[start]


def returned(value):
    return int(value) if value is not None and value.isdigit() else 0


# prints: the variable before, after, whether anything else in the environment changed, the value returned, library loaded?
PY_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
before = dict(os.environ)
import rsicnv_amd.api as api
after = dict(os.environ)
rest = {k: v for k, v in before.items() if k != "GPU_MAX_HW_QUEUES"} == {k: v for k, v in after.items() if k != "GPU_MAX_HW_QUEUES"}
print(repr((before.get("GPU_MAX_HW_QUEUES"), after.get("GPU_MAX_HW_QUEUES"), rest, api.HW_QUEUES, api._lib is not None)))
"""
# the C function changes the C environment, which os.environ does not re-read: ask getenv
C_CHILD = r"""
import ctypes, sys
libc = ctypes.CDLL(None)
libc.getenv.restype = ctypes.c_char_p
libc.getenv.argtypes = [ctypes.c_char_p]
get = lambda k: (lambda v: None if v is None else v.decode())(libc.getenv(k))
before = (get(b"GPU_MAX_HW_QUEUES"), get(b"RSI_HOT_HW_QUEUES"))
lib = ctypes.CDLL(sys.argv[1])
lib.rsi_hot_process_setup.argtypes = []
lib.rsi_hot_process_setup.restype = ctypes.c_int
rc = lib.rsi_hot_process_setup()
again = lib.rsi_hot_process_setup()
print(repr((before[0], get(b"GPU_MAX_HW_QUEUES"), before[1] == get(b"RSI_HOT_HW_QUEUES"), rc, again)))
"""


def child(script, arg, start, user):
    env = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "RSI_HOT_HW_QUEUES")}
    if start is not None:
        env["GPU_MAX_HW_QUEUES"] = start
    if user is not None:
        env["RSI_HOT_HW_QUEUES"] = user
    r = subprocess.run([sys.executable, "-c", script, arg], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-600:]
    return eval(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def outcomes():
    """{(path, start, user): the child's tuple}: every child once, four at a time."""
    assert os.path.exists(LIB), "build with make -f rsicnv_amd/csrc/Makefile"
    cases = [(s, u) for s in STARTS for u in USERS] + [(s, None) for s, _ in ODD_STARTS]
    jobs = [(path, s, u) for s, u in cases for path in ("py", "c")]
    with ThreadPoolExecutor(max_workers=4) as ex:
        got = list(ex.map(lambda j: child(PY_CHILD, ROOT, j[1], j[2]) if j[0] == "py" else child(C_CHILD, LIB, j[1], j[2]), jobs))
    return dict(zip(jobs, got))


@pytest.mark.parametrize("user", USERS, ids=lambda u: f"user_{u}")
@pytest.mark.parametrize("start", STARTS, ids=lambda s: f"start_{s}")
def test_policy(outcomes, start, user):
    want = expected(start, user)
    before, after, rest_same, value, lib_loaded = outcomes[("py", start, user)]
    assert before == start
    assert after == want, f"import rsicnv_amd.api: GPU_MAX_HW_QUEUES {start!r} with RSI_HOT_HW_QUEUES {user!r} became {after!r}, not {want!r}"
    assert rest_same and value == returned(want)
    assert not lib_loaded, "the import must not load librsi_hot.so"
    c_before, c_after, user_same, rc, again = outcomes[("c", start, user)]
    assert c_before == start
    assert c_after == want, f"rsi_hot_process_setup: GPU_MAX_HW_QUEUES {start!r} with RSI_HOT_HW_QUEUES {user!r} became {c_after!r}, not {want!r}"
    assert user_same and rc == returned(want) and again == rc   # a second call finds its own answer and keeps it
    if after is not None and after != start:   # whatever is written lies in 4 .. 32
        assert 4 <= int(after) <= 32


def test_the_cases_the_policy_names(outcomes):
    for path in ("py", "c"):
        assert outcomes[(path, "4", None)][1] == "32"
        assert outcomes[(path, "64", None)][1] == "64" and outcomes[(path, "64", "keep")][1] == "64"
        assert outcomes[(path, "64", "99")][1] == "32"      # the user's number is clamped, never written above 32
        assert outcomes[(path, "2", "2")][1] == "4"
        for start in STARTS:
            assert outcomes[(path, start, "keep")][1] == start


@pytest.mark.parametrize("start,want", ODD_STARTS, ids=[repr(s) for s, _ in ODD_STARTS])
def test_what_counts_as_a_number(outcomes, start, want):
    py, c = outcomes[("py", start, None)], outcomes[("c", start, None)]
    assert py[1] == want and c[1] == want
    assert py[3] == c[3] == int(want)
