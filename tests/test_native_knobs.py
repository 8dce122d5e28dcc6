"""What each native environment switch does to the host policy, through the queries ``_C`` exports (CPU: the
policy is host code in the extension). Every switch is one ``dla::Knob`` (csrc/include/dla_knob.h); this pins,
per query, the answer with the knob unset, set to a non-default in the environment, and overridden then cleared
through its ``set_*`` function -- clearing always returns to the environment's value, never to the literal
default. The environment is read once per process, so each environment gets one fresh child process, which
answers every query in one go.

The recorded answers are those of the code before the switches were moved onto ``dla::Knob``, except the two
marked "changed": ``set_tile256_min_k_stats(-1)`` and ``set_gemm_apply_max_k(-1)`` used to forget
``DLA_TILE256_MIN_K_STATS`` / ``DLA_APPLY_MAX_K`` and go back to 256 / 512. (``pick_tile``'s ``stats`` argument
came with that change: without it no query showed the statistics forwards' threshold.)"""
import functools
import json
import os
import subprocess
import sys

import pytest

from distributed_learning_amd.ops import _ext

pytestmark = pytest.mark.skipif(not _ext.available(), reason="native extension not built")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T128, T256, T512x128 = 1, 8, 9

# (name, expression over C) in the order the child evaluates them; a setter returns None, so `or` chains to the query
STEPS = [
    # TILE256 / TILE512 (no setters)
    ("tile", "C.pick_tile(100352, 256, 2304, True)"),
    ("conv_tile", "C.pick_conv_tile(1003520, 128, 1152, True)"),
    # TILE256_MIN_K_STATS: the statistics forwards' smallest K for 256x256 tiles (s14 conv3 forward, K = 256)
    ("tile_stats", "C.pick_tile(100352, 1024, 256, True, True)"),
    ("tile_stats_set", "C.set_tile256_min_k_stats(1024) or C.pick_tile(100352, 1024, 256, True, True)"),
    ("tile_stats_cleared", "C.set_tile256_min_k_stats(-1) or C.pick_tile(100352, 1024, 256, True, True)"),
    # TN256: 256x256 weight-gradient tiles (also off under TILE256=0)
    ("tn", "C.gemm_tn_splits(1024, 256, 100352)"),
    ("tn_off", "C.set_tn256(0) or C.gemm_tn_splits(1024, 256, 100352)"),
    ("tn_on", "C.set_tn256(1) or C.gemm_tn_splits(1024, 256, 100352)"),
    ("tn_cleared", "C.set_tn256(-1) or C.gemm_tn_splits(1024, 256, 100352)"),
    # SPLITK_BLOCKS
    ("splitk", "[C.splitk_target_blocks(), C.gemm_tn_splits(128, 512, 401408)]"),
    ("splitk_set", "C.set_splitk_blocks(128) or [C.splitk_target_blocks(), C.gemm_tn_splits(128, 512, 401408)]"),
    ("splitk_cleared", "C.set_splitk_blocks(0) or [C.splitk_target_blocks(), C.gemm_tn_splits(128, 512, 401408)]"),
    # BN_RED_BLOCKS
    ("red", "C.bn_red_blocks()"),
    ("red_set", "C.set_bn_red_blocks(64) or C.bn_red_blocks()"),
    ("red_cleared", "C.set_bn_red_blocks(0) or C.bn_red_blocks()"),
    # HALO (no setter): [forward, data gradient]
    ("halo", "[C.halo_conv_eligible(64, 64, 56, 1, True), C.halo_conv_eligible(64, 64, 56, 1, False)]"),
    # HALO_WGRAD
    ("halo_wgrad", "C.halo_wgrad_eligible(64, 64, 56, 1)"),
    ("halo_wgrad_off", "C.set_halo_wgrad(0) or C.halo_wgrad_eligible(64, 64, 56, 1)"),
    ("halo_wgrad_on", "C.set_halo_wgrad(1) or C.halo_wgrad_eligible(64, 64, 56, 1)"),
    ("halo_wgrad_cleared", "C.set_halo_wgrad(-1) or C.halo_wgrad_eligible(64, 64, 56, 1)"),
    # POOL3_SEP: strip height of the 3x3/s1 max-pool forward (4 or 7; anything else: the generic kernel)
    ("pool3", "C.pool3_strip_rows()"),
    ("pool3_7", "C.set_pool3_sep(7) or C.pool3_strip_rows()"),
    ("pool3_off", "C.set_pool3_sep(0) or C.pool3_strip_rows()"),
    ("pool3_other", "C.set_pool3_sep(5) or C.pool3_strip_rows()"),
    ("pool3_cleared", "C.set_pool3_sep(-1) or C.pool3_strip_rows()"),
    # APPLY_MAX_K (capped at 2048): K = 512, 1024, 2048, 4096
    ("apply", "[C.gemm_nt_apply_ok(4096, 64, k) for k in (512, 1024, 2048, 4096)]"),
    ("apply_set", "C.set_gemm_apply_max_k(256) or [C.gemm_nt_apply_ok(4096, 64, k) for k in (256, 512)]"),
    ("apply_set_cap", "C.set_gemm_apply_max_k(1 << 20) or [C.gemm_nt_apply_ok(4096, 64, k) for k in (2048, 4096)]"),
    ("apply_cleared", "C.set_gemm_apply_max_k(-1) or [C.gemm_nt_apply_ok(4096, 64, k) for k in (512, 1024, 2048, 4096)]"),
    # GEMM_STREAM: statistics rows at K = 64 (forward), K = 256 forward / data gradient (k-major); forced on
    # (set_gemm_stream(1)) also serves the K = 256 forward, on by default or by the environment does not
    ("stream", "[C.gemm_stream_rows(802816, 256, 64, 64, 256), C.gemm_stream_rows(802816, 512, 256, 256, 512), "
               "C.gemm_stream_rows(802816, 512, 256, 256, 512, True), C.gemm_nt_stream_apply_ok(802816, 256, 64)]"),
    ("stream_off", "C.set_gemm_stream(0) or [C.gemm_stream_rows(802816, 256, 64, 64, 256), "
                   "C.gemm_stream_rows(802816, 512, 256, 256, 512, True), C.gemm_nt_stream_apply_ok(802816, 256, 64)]"),
    ("stream_forced", "C.set_gemm_stream(1) or [C.gemm_stream_rows(802816, 256, 64, 64, 256), "
                      "C.gemm_stream_rows(802816, 512, 256, 256, 512), C.gemm_nt_stream_apply_ok(802816, 256, 64)]"),
    ("stream_cleared", "C.set_gemm_stream(-1) or [C.gemm_stream_rows(802816, 256, 64, 64, 256), "
                       "C.gemm_stream_rows(802816, 512, 256, 256, 512), "
                       "C.gemm_stream_rows(802816, 512, 256, 256, 512, True), C.gemm_nt_stream_apply_ok(802816, 256, 64)]"),
]

_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
from distributed_learning_amd.ops import _ext
C = _ext.require()
out = {}
for name, expr in json.loads(sys.argv[2]):
    try:
        out[name] = eval(expr)
    except Exception as e:  # reported as the answer, so one bad step does not hide the others
        out[name] = f"{type(e).__name__}: {e}"
print("ANSWERS " + json.dumps(out))
"""

DEFAULTS = {
    "tile": T256, "conv_tile": T512x128,
    "tile_stats": T256, "tile_stats_set": T128, "tile_stats_cleared": T256,
    "tn": 64, "tn_off": 32, "tn_on": 64, "tn_cleared": 64,
    "splitk": [512, 128], "splitk_set": [128, 32], "splitk_cleared": [512, 128],
    "red": 1024, "red_set": 64, "red_cleared": 1024,
    "halo": [True, True],
    "halo_wgrad": True, "halo_wgrad_off": False, "halo_wgrad_on": True, "halo_wgrad_cleared": True,
    "pool3": 4, "pool3_7": 7, "pool3_off": 0, "pool3_other": 0, "pool3_cleared": 4,
    "apply": [True, False, False, False], "apply_set": [True, False], "apply_set_cap": [True, False],
    "apply_cleared": [True, False, False, False],
    "stream": [128, 0, 64, True], "stream_off": [0, 0, False], "stream_forced": [128, 64, True],
    "stream_cleared": [128, 0, 64, True],
}

# environment -> the answers that differ from DEFAULTS there
CASES = {
    "unset": ({}, {}),
    "non_default": (
        {"DLA_TILE512": "0", "DLA_TILE256_MIN_K_STATS": "512", "DLA_TN256": "0", "DLA_SPLITK_BLOCKS": "256",
         "DLA_BN_RED_BLOCKS": "300", "DLA_HALO": "1", "DLA_HALO_WGRAD": "0", "DLA_APPLY_MAX_K": "1024",
         "DLA_GEMM_STREAM": "0", "DLA_POOL3_SEP": "7"},
        {"conv_tile": T128,
         "pool3": 7, "pool3_cleared": 7,
         "tile_stats": T128, "tile_stats_cleared": T128,  # changed: the setter's -1 used to give T256 (min K 256)
         "tn": 16, "tn_off": 16, "tn_on": 32, "tn_cleared": 16,  # half of the defaults': SPLITK_BLOCKS=256
         "splitk": [256, 64], "splitk_cleared": [256, 64],
         "red": 300, "red_cleared": 300,
         "halo": [False, True],
         "halo_wgrad": False, "halo_wgrad_cleared": False,
         "apply": [True, True, False, False],
         "apply_cleared": [True, True, False, False],  # changed: the setter's -1 used to give max K 512
         "stream": [0, 0, 0, False], "stream_cleared": [0, 0, 0, False]},
    ),
    "tile256_off": (
        {"DLA_TILE256": "0"},
        {"tile": T128, "conv_tile": T128, "tile_stats": T128, "tile_stats_cleared": T128,
         "tn": 32, "tn_on": 32, "tn_cleared": 32},
    ),
    "other_values": (
        # HALO off; GEMM_STREAM on by the environment is not "forced on"; APPLY_MAX_K above its cap; switches
        # parse the first character only
        {"DLA_HALO": "0", "DLA_GEMM_STREAM": "1", "DLA_APPLY_MAX_K": "4096", "DLA_TN256": "off",
         "DLA_HALO_WGRAD": "00", "DLA_SPLITK_BLOCKS": "-3", "DLA_BN_RED_BLOCKS": "abc", "DLA_POOL3_SEP": "0"},
        {"halo": [False, False],
         "pool3": 0, "pool3_cleared": 0,
         "halo_wgrad": False, "halo_wgrad_cleared": False,
         "apply": [True, True, True, False], "apply_cleared": [True, True, True, False]},
    ),
}


@functools.lru_cache(maxsize=None)
def _answers(case):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DLA_")}
    env.update(CASES[case][0])
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(STEPS)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ANSWERS ")][-1]
    return json.loads(line[len("ANSWERS "):])


@pytest.mark.parametrize("step", [name for name, _ in STEPS])
@pytest.mark.parametrize("case", list(CASES))
def test_knob_policy(case, step):
    want = dict(DEFAULTS, **CASES[case][1])[step]
    assert _answers(case)[step] == want, f"{dict(STEPS)[step]} under {CASES[case][0] or 'no DLA_* variable'}"


def test_every_case_names_known_steps():
    names = {n for n, _ in STEPS}
    assert set(DEFAULTS) == names
    for env, diff in CASES.values():
        assert set(diff) <= names
