"""The option table of libpsa_hip.so (psa_option_info) against the header that documents it and the Python constants
that name it, and the process-wide count of device buffers before any context exists.  No GPU."""
import ctypes
import re
import subprocess
import sys
from pathlib import Path

from psa_amd import _hip

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "psa_hip.h").read_text()
IDS = list(range(14)) + [15]


def _documented_defaults():
    """name -> the [default] of the header's comment block, as bytes or a plain number"""
    out = {}
    for name, num, unit in re.findall(r"^\s*/?\*\s+(PSA_OPT_\w+)\s+\[(\d+)(?: (KiB|MiB|GiB))?\]", HEADER, flags=re.M):
        assert name not in out, name
        out[name] = int(num) << {"": 0, "KiB": 10, "MiB": 20, "GiB": 30}[unit]
    return out


def test_table_lists_exactly_the_options_of_the_header():
    table = _hip.option_table()
    assert [row[0] for row in table] == IDS
    defines = {n: int(v) for n, v in re.findall(r"^#define\s+(PSA_OPT_\w+)\s+(\d+)", HEADER, flags=re.M)}
    assert {name: opt for opt, name, _ in table} == defines
    constants = {n: v for n, v in vars(_hip).items() if n.startswith("OPT_")}
    assert {name[len("PSA_"):]: opt for opt, name, _ in table} == constants


def test_every_documented_default_is_the_tables():
    table = {name: default for _, name, default in _hip.option_table()}
    documented = _documented_defaults()
    assert documented == table
    assert documented["PSA_OPT_K1_WIDE"] == 1 and documented["PSA_OPT_PLANES_MIN_K"] == 17
    assert documented["PSA_OPT_K1_LOWRANK_MIN_K"] == 256 and documented["PSA_OPT_VDOS_WORK_BYTES"] == 1 << 30
    assert documented["PSA_OPT_DYNAMIC_WORK_BYTES"] == 4 << 30


def test_past_the_end_is_einval():
    lib = _hip.load_library()
    opt, default, name = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_char_p()
    args = (ctypes.byref(opt), ctypes.byref(default), ctypes.byref(name))
    assert lib.psa_option_info(len(IDS) - 1, *args) == 0 and opt.value == 15
    assert lib.psa_option_info(len(IDS), *args) == -1 and b"no option at index 15" in lib.psa_last_error()
    assert lib.psa_option_info(-1, *args) == -1
    assert lib.psa_option_info(0, None, None, None) == 0                     # any output may be null


def test_no_context_no_device_buffers():
    """in a process of its own: no context was ever created there"""
    code = "from psa_amd import _hip; assert _hip.device_buffers() == (0, 0), _hip.device_buffers()"
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
