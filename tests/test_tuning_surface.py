"""The tuning surface of the library without a GPU: which knobs `ec_tune_set` accepts, that `ec_stat_get("tune.<knob>")` reads each one
back, and the written spec of what every knob holds after any int64 value — the value read back is the value the launchers act on.
Out-of-range values saturate into the documented range or are refused with the knob unchanged; nothing wraps through int.  The cells
the kernels compute under every accepted value are checked on the GPU (tests/test_gpu_tuning_knobs.py)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "erased-cells_amd", "python"))
import erased_cells_hip as ec  # noqa: E402

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

# The `Tuning` initialisers of csrc/ec_runtime.hpp, written here once: a changed default has to be changed in both places on purpose.
DEFAULTS = {
    "binop_variant": -1, "reduce_bpc": 0, "reduce_shape": 0, "map_u": 2, "peel": 1, "unaligned_vector": 1, "fused_mixed": 1,
    "mall_mb": 256, "inject_shard_failure": 0, "inject_pin_refusal": 0, "expr_jit": 1, "expr_fixed": 1, "write_lds_kb": 64,
    "binop_lds_kb": -1, "scalar_lds_kb": -1, "map_lds_kb": 0, "fused_lds_kb": 0, "counts_one_launch": 1, "cache_force": -1,
    "pool_keep_mb": 32768,
}

# The spec, per knob: (documented values, accepted range [lo, hi], what a value outside the range does).
#   "clamp"  saturates to the nearer end; "refuse": EC_ERR_ARG, the knob unchanged; "bool": stores value != 0.
# A value inside [lo, hi] but not documented (map_u = 3) is refused.
SPEC = {
    "binop_variant": ([-1, 0, 1], -1, 1, "refuse"),
    "reduce_bpc": ([0, 1, 2, 16, 4096], 0, 4096, "clamp"),
    "reduce_shape": ([0, 1, 2, 3, 4], 0, 4, "refuse"),
    "map_u": ([1, 2, 4], 1, 4, "refuse"),
    "peel": ([0, 1, 2], 0, 2, "refuse"),
    "unaligned_vector": ([0, 1], 0, 1, "bool"),
    "fused_mixed": ([0, 1], 0, 1, "bool"),
    "mall_mb": ([0, 3, 256, 1 << 20], 0, 1 << 20, "clamp"),
    "inject_shard_failure": ([0, 1, 2], 0, (1 << 31) - 1, "refuse"),
    "inject_pin_refusal": ([0, 1], 0, 1, "bool"),
    "expr_jit": ([0, 1, 2], 0, 2, "clamp"),
    "expr_fixed": ([0, 1], 0, 1, "bool"),
    "write_lds_kb": ([0, 32, 64], 0, 64, "clamp"),
    "binop_lds_kb": ([-1, 0, 1, 16, 32, 48, 64], -1, 64, "clamp"),
    "scalar_lds_kb": ([-1, 0, 32, 64], -1, 64, "clamp"),
    "map_lds_kb": ([0, 16, 64], 0, 64, "clamp"),
    "fused_lds_kb": ([0, 16, 64], 0, 64, "clamp"),
    "counts_one_launch": ([0, 1, 2], 0, 2, "clamp"),
    "cache_force": ([-1, 0, 1, 5, 15, 255], -1, 255, "refuse"),
    "pool_keep_mb": ([0, 32768, 1 << 20], 0, 1 << 20, "clamp"),
}
REFUSED_INSIDE = {"map_u": {3}}


def expected(knob, value):
    """What `tune.<knob>` reads after ec_tune_set(knob, value): an int, or None when the call must be refused."""
    documented, lo, hi, rule = SPEC[knob]
    if rule == "bool":
        return int(value != 0)
    if value in REFUSED_INSIDE.get(knob, ()):
        return None
    if lo <= value <= hi:
        return value
    return None if rule == "refuse" else (lo if value < lo else hi)


def probes(knob):
    documented, lo, hi, _ = SPEC[knob]
    return sorted(set(documented) | {lo, hi, lo - 1, hi + 1, 0, -1, 1 << 31, (1 << 32) + 1, 1 << 32, I64_MIN, I64_MAX})


def read(key):
    v = C.c_int64(-12345)
    st = ec.lib().ec_stat_get(b"tune." + key.encode(), C.byref(v))
    assert st == ec._ffi.EC_OK, (key, st, ec.lib().ec_last_error_string())
    return v.value


def snapshot():
    return {k: read(k) for k in DEFAULTS}


@pytest.fixture(autouse=True)
def restore_every_knob():
    """Every knob as it was before the test, and checked to be so afterwards."""
    before = snapshot()
    yield
    for k, v in before.items():
        assert ec.lib().ec_tune_set(k.encode(), v) == ec._ffi.EC_OK
    assert snapshot() == before


def _runtime_keys():
    src = open(os.path.join(ROOT, "erased-cells_amd", "csrc", "ec_runtime.hip")).read()
    table = src[src.index("const Knob kKnobs[] = {"):]
    table = table[:table.index("};")]
    entries = re.findall(r'\{"(\w+)", (?:&g_tuning\.(\w+), nullptr|nullptr, &g_tuning\.(\w+))', table)
    for key, fi, fl in entries:
        assert key == (fi or fl), f"ec_tune_set key {key!r} writes the field {fi or fl!r}"
    return [e[0] for e in entries]


def _header_keys():
    h = open(os.path.join(ROOT, "include", "erased_cells.h")).read()
    decl = h.index("ec_status ec_tune_set(const char *key, int64_t value);")
    comment = h[h.rindex("/*", 0, decl):decl]
    return re.findall(r'"([a-z_0-9]+)"', comment)


def test_the_keys_accepted_are_the_keys_documented():
    runtime, header = _runtime_keys(), _header_keys()
    assert len(runtime) == len(set(runtime)) and len(header) == len(set(header))
    assert set(runtime) == set(header)
    assert set(runtime) == set(DEFAULTS) == set(SPEC), "the test's own tables name every knob"


def test_every_knob_reads_back():
    for key in DEFAULTS:
        read(key)
    v = C.c_int64()
    assert ec.lib().ec_stat_get(b"tune.no_such_knob", C.byref(v)) == ec._ffi.EC_ERR_ARG
    assert ec.lib().ec_tune_set(b"no_such_knob", 1) == ec._ffi.EC_ERR_ARG
    assert ec.lib().ec_tune_set(None, 1) == ec._ffi.EC_ERR_ARG


@pytest.mark.parametrize("knob", sorted(SPEC))
def test_the_value_read_back_follows_the_spec(knob):
    L, E = ec.lib(), ec._ffi
    for v in probes(knob):
        # start each probe from a documented value other than the expected answer, so that "unchanged" is visible
        documented = SPEC[knob][0]
        want = expected(knob, v)
        start = next((d for d in documented if d != want), documented[0])
        assert L.ec_tune_set(knob.encode(), start) == E.EC_OK and read(knob) == start
        st = L.ec_tune_set(knob.encode(), v)
        if want is None:
            assert st == E.EC_ERR_ARG, (knob, v, read(knob))
            assert knob.encode() in L.ec_last_error_string()
            assert read(knob) == start, f"{knob} = {v} refused, but the knob changed"
        else:
            assert st == E.EC_OK, (knob, v, L.ec_last_error_string())
            assert read(knob) == want, (knob, v, read(knob), want)


def test_the_values_that_used_to_wrap():
    """Literal cases, independent of the SPEC helper: each was stored through a narrowing to int (or as given) before."""
    L, E = ec.lib(), ec._ffi
    cases = [("reduce_bpc", (1 << 32) + 1, 4096), ("reduce_bpc", 1 << 31, 4096), ("peel", 1 << 32, None), ("peel", 7, None),
             ("cache_force", 1 << 32, None), ("map_u", 3, None), ("reduce_shape", 9, None), ("binop_variant", 5, None),
             ("binop_lds_kb", 65, 64), ("binop_lds_kb", I64_MIN, -1), ("map_lds_kb", -1, 0), ("fused_mixed", 1 << 32, 1),
             ("mall_mb", I64_MAX, 1 << 20), ("pool_keep_mb", I64_MAX, 1 << 20), ("inject_shard_failure", 1 << 32, None),
             ("inject_pin_refusal", 1 << 32, 1), ("expr_fixed", 1 << 32, 1), ("counts_one_launch", I64_MAX, 2)]
    for knob, v, want in cases:
        before = read(knob)
        st = L.ec_tune_set(knob.encode(), v)
        if want is None:
            assert st == E.EC_ERR_ARG and read(knob) == before, (knob, v)
        else:
            assert st == E.EC_OK and read(knob) == want, (knob, v, read(knob))
        assert L.ec_tune_set(knob.encode(), before) == E.EC_OK


def test_a_fresh_process_reads_the_shipped_defaults():
    code = ("import ctypes as C, json, sys; sys.path.insert(0, sys.argv[1]); import erased_cells_hip as ec\n"
            "v = C.c_int64(); out = {}\n"
            "for k in sys.argv[2:]:\n"
            "    assert ec.lib().ec_stat_get(b'tune.' + k.encode(), C.byref(v)) == 0, k\n"
            "    out[k] = v.value\n"
            "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "erased-cells_amd", "python"), *DEFAULTS],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == DEFAULTS


def test_tuned_sets_and_puts_back():
    before = snapshot()
    with ec.tuned(binop_variant=1, map_u=4, reduce_bpc=(1 << 32) + 1):
        assert (read("binop_variant"), read("map_u"), read("reduce_bpc")) == (1, 4, 4096)
        with ec.tuned(map_u=1, binop_lds_kb=48):
            assert (read("map_u"), read("binop_lds_kb"), read("binop_variant")) == (1, 48, 1)
        assert (read("map_u"), read("binop_lds_kb")) == (4, before["binop_lds_kb"])
    assert snapshot() == before
    # a refused value raises with every knob as it was, including those named before it
    with pytest.raises(ec.EcError, match="map_u"):
        with ec.tuned(binop_variant=0, map_u=3):
            pass
    assert snapshot() == before
    with pytest.raises(ec.EcError, match="no_such_knob"):
        with ec.tuned(no_such_knob=1):
            pass
    # an exception inside the block still restores
    with pytest.raises(RuntimeError):
        with ec.tuned(peel=2):
            raise RuntimeError("inside")
    assert snapshot() == before
