"""The training schedule's shared state machine (csrc/qcart_sched.hpp) without a GPU: a stand-alone program
(tests/diag/sched_check.cpp, its own main, built with -ffp-contract=off and AddressSanitizer + UBSan, run as a plain
executable) reads scripted tick sequences, runs the functions the kernel runs and prints the snapshots; they are
compared by bit pattern with the plain-Python restatement tests/sched_ref.py. The scripts reach every branch (each
branch counter of the reference is asserted non-zero). Also: the parameter refusals with their texts, the kSched
state header through qcart_state.hpp's validator, and the new entry points in the header, the binding and the
library."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from deepreinforcementlearningcontrolofquantumcartpoles_amd import _lib
from tests import sched_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "diag", "sched_check.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("sched_check")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run([cxx, *flags, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0 \
            or subprocess.run([str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot build or run -fsanitize=address,undefined programs here")
    out = tmp / "sched_check"
    subprocess.run([cxx, *flags, "-Wall", "-Wextra", "-Werror", SRC, "-o", str(out)], check=True)
    return str(out)


def run(exe, mode, text, tmp_path):
    path = tmp_path / "script.txt"
    path.write_text(text)
    r = subprocess.run([exe, mode, str(path)], capture_output=True, text=True, timeout=120)
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    return r


def parse_line(line: str) -> tuple:
    vals = []
    for w, f in zip(line.split(), R.SNAP_LINE):
        v = int(w, 16) if f == "d" else int(w)
        vals.append(v - (1 << 64) if f == "d" and v >= 1 << 63 else v)
    return tuple(vals)


@pytest.fixture(scope="module")
def reference_runs():
    """Each script through the reference, once: (snapshots as bit tuples, branch counters)."""
    out = {}
    for name, (p, cap, ticks) in R.scripts().items():
        ref = R.SchedRef(p)
        out[name] = ([R.snapshot_bits(ref.tick(ts, rows, cap)) for rows, ts in ticks], ref.hits)
    return out


@pytest.mark.parametrize("name", sorted(R.scripts()))
def test_state_machine_equals_the_reference_bit_for_bit(exe, reference_runs, tmp_path, name):
    p, cap, ticks = R.scripts()[name]
    r = run(exe, "run", R.script_text(p, cap, ticks), tmp_path)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    got = [parse_line(ln) for ln in r.stdout.splitlines()]
    want = reference_runs[name][0]
    assert len(got) == len(want) == len(ticks)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, i, dict(zip(R.SNAPSHOT_FIELDS, g)), dict(zip(R.SNAPSHOT_FIELDS, w)))


def test_the_scripts_reach_every_branch(reference_runs):
    hits = sum((h for _, h in reference_runs.values()), start=type(reference_runs["cartpole"][1])())
    for branch in ("cartpole_start", "cartpole_fall", "cartpole_restart",
                   "cooling_first_full", "cooling_reset_at_limit_minus_one", "cooling_counter_reset",
                   "cooling_fail_limit", "cooling_better", "zero_sample",
                   "lr_cap", "lr_step", "lr_steps_consecutive", "backup_switch",
                   "rung0", "rung1", "rung2", "rung3", "push", "push_not_started", "save", "save_waits_for_push",
                   "stop_done", "stop_give_up", "updates_capped", "min_rows_hold", "train0"):
        assert hits[branch] > 0, branch
    assert reference_runs["cartpole"][1]["backup_switch"] == 1            # the period switches once
    assert reference_runs["cooling"][1]["cooling_first_full"] == 2        # and again after learning was cleared
    # what the cases are about, in the snapshots themselves
    snaps = [dict(zip(R.SNAPSHOT_FIELDS, s)) for s in reference_runs["cartpole"][0]]
    assert {s["backup_period"] for s in snaps} == {100, 3}
    assert any(s["n_updates"] == 0 and s["total_rows"] > 0 for s in snaps[:1])    # min_rows
    assert max(s["n_updates"] for s in snaps) == 2 and any(s["push"] and not s["save"] for s in snaps)
    assert all(s["push"] for s in snaps if s["save"])
    test = [dict(zip(R.SNAPSHOT_FIELDS, s)) for s in reference_runs["test_mode"][0]]
    assert all(s["n_updates"] == s["push"] == s["save"] == 0 for s in test) and test[-1]["n"] == 14
    assert test[0]["learning"] == 0 and test[1]["learning"] == 1          # set at the first episode


def test_sem_equals_numpy_on_the_test_mode_script(reference_runs):
    """mean and sem come from running sums (count, sum, sum of squares), numpy's from two passes: they agree to the
    rounding of the sums. Bound: the n + 2 roundings of each sum, relative 2^-53 each, amplified for the variance by
    sumsq / (sumsq - sum^2 / n)."""
    import numpy as np
    import struct
    p, cap, ticks = R.scripts()["test_mode"]
    ts = np.array([t for _, tt in ticks for t in tt])
    last = dict(zip(R.SNAPSHOT_FIELDS, reference_runs["test_mode"][0][-1]))
    mean, sem = (struct.unpack("<d", struct.pack("<q", last[k]))[0] for k in ("mean", "sem"))
    n, eps = len(ts), 2.0 ** -53
    assert last["n"] == n
    assert abs(mean - ts.mean()) <= (n + 2) * eps * abs(ts.mean())
    amp = (ts ** 2).sum() / ((ts ** 2).sum() - ts.sum() ** 2 / n)
    want = ts.std(ddof=1) / np.sqrt(n)
    assert abs(sem - want) <= (n + 4) * eps * amp * want


REFUSALS = [
    (dict(rule=2), "rule must be QC_SCHED_CARTPOLE or QC_SCHED_COOLING"),
    (dict(train=2), "train must be 0 or 1"),
    (dict(fall_time=0.), "fall_time must be > 0"),
    (dict(start_time=5., fall_time=5.), "start_time must be above fall_time"),
    (dict(start_time=float("inf")), "start_time must be finite"),
    (dict(rule=R.COOLING, t_full=0.), "t_full must be finite and > 0"),
    (dict(rule=R.COOLING, t_full=10., fail_limit=0), "fail_limit must be >= 1"),
    (dict(rule=R.COOLING, t_full=10., first_interval_time=7.),
     "first_interval_time must be >= 0 and 1.5 first_interval_time below t_full"),
    (dict(batch_size=0), "batch_size must be >= 1"),
    (dict(n_times_per_sample=0.), "n_times_per_sample must be finite and > 0"),
    (dict(max_updates_per_tick=0), "max_updates_per_tick must be >= 1"),
    (dict(min_rows=-1), "min_rows must be >= 0"),
    (dict(num_episodes=0), "num_episodes must be >= 1"),
    (dict(give_up_episodes=-1), "give_up_episodes must be >= 0"),
    (dict(lr_init=-1e-4), "lr_init must be finite and >= 0"),
    (dict(lr_cap=0.), "lr_cap must be > 0"),
    (dict(lr_schedule=tuple((i, 1e-4) for i in range(9))), "lr_schedule holds at most 8 pairs"),
    (dict(lr_schedule=((10, 1e-4), (10, 1e-5))), "lr_schedule episodes must be strictly increasing"),
    (dict(lr_schedule=((-1, 1e-4),)), "lr_schedule episodes must be >= 0"),
    (dict(lr_schedule=((10, float("nan")),)), "lr_schedule rates must be finite and >= 0"),
    (dict(backup_period=0), "backup_period and warm_backup_period must be >= 1"),
    (dict(warm_backup_period=0), "backup_period and warm_backup_period must be >= 1"),
    (dict(save_interval=0), "save_interval must be >= 1"),
    (dict(actor_update_time=0.), "actor_update_time must be finite and > 0"),
    (dict(rungs=R.IHO_RUNGS + ((1., 2., 3.),)), "scale_up_actor_update_time has at most 4 rungs"),
    (dict(rungs=((5., 10., 10.),)), "a rung needs achieved >= 0, below > 0 and a time above below"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[t[:40] + "-" + "-".join(k) for k, t in REFUSALS])
def test_parameter_refusals_with_their_texts(exe, tmp_path, kw, text):
    r = run(exe, "params", R.script_text(R.params(**kw), 128, []), tmp_path)
    assert r.returncode == 0 and r.stdout.strip() == text
    # and a refused script does not run
    r = run(exe, "run", R.script_text(R.params(**kw), 128, [(1, [1.])]), tmp_path)
    assert r.returncode == 2 and r.stdout.strip() == "refused: " + text


def test_the_drivers_params_are_accepted(exe, tmp_path):
    assert run(exe, "params", R.script_text(R.params(), 128, []), tmp_path).stdout.strip() == "ok"
    for name, (p, cap, _) in R.scripts().items():
        assert run(exe, "params", R.script_text(p, cap, []), tmp_path).stdout.strip() == "ok", name


@pytest.mark.parametrize("name", ["cartpole", "cooling"])
def test_sched_state_header_through_the_validator(exe, tmp_path, name):
    """Every truncation and one corruption per header word and per field of a kSched blob is refused, with the
    field's name; a schedule or rung table that differs in one entry is refused by its hash."""
    p, cap, _ = R.scripts()[name]
    r = run(exe, "header", R.script_text(p, cap, []), tmp_path)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-2000:], r.stderr[-2000:])


def test_new_entry_points_in_header_binding_and_library():
    names = ["qc_sched_create", "qc_sched_destroy", "qc_sched_last_error", "qc_sched_set_stream", "qc_sched_tick",
             "qc_sched_poll", "qc_sched_seek", "qc_sched_state_bytes", "qc_sched_state_export", "qc_sched_state_import",
             "qc_learner_set_backup_period", "qc_mlearner_set_backup_period"]
    assert set(names) <= set(_lib.EXPORTS) and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    header = open(os.path.join(ROOT, "include", "qcart.h")).read()
    for n in names:
        assert re.search(rf"\b{n}\(", header), n
    if os.path.exists(_lib.LIB_PATH):
        so = ctypes.CDLL(_lib.LIB_PATH)
        for n in names:
            assert hasattr(so, n), n


def test_structs_match_the_header(tmp_path):
    """_lib.QcSchedParams and _lib.QcSchedSnapshot mirror the C structs: offsets and sizes compiled against the header."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    for cname, cls in (("qc_sched_params", _lib.QcSchedParams), ("qc_sched_snapshot", _lib.QcSchedSnapshot)):
        names = [f[0] for f in cls._fields_]
        src = tmp_path / f"{cname}.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qcart.h"\nint main(void){\n'
                       + "".join(f'printf("%zu\\n", offsetof({cname}, {n}));\n' for n in names)
                       + f'printf("%zu\\n", sizeof({cname}));return 0;}}\n')
        exe_ = tmp_path / cname
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe_)], check=True)
        got = [int(v) for v in subprocess.run([str(exe_)], check=True, capture_output=True, text=True).stdout.split()]
        assert got == [getattr(cls, n).offset for n in names] + [ctypes.sizeof(cls)], cname
    assert [f[0] for f in _lib.QcSchedSnapshot._fields_] == list(R.SNAPSHOT_FIELDS)


def test_cli_refuses_more_than_one_rank():
    """python -m <package>.train has no multi-GPU path: WORLD_SIZE > 1 is refused before any device is touched."""
    import sys
    env = dict(os.environ, WORLD_SIZE="2")
    r = subprocess.run([sys.executable, "-m", "deepreinforcementlearningcontrolofquantumcartpoles_amd.train",
                        "--system", "iho"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE > 1 is refused" in r.stderr
