"""tests/gpu_child.py, the suite's one runner of child processes, on the CPU: which ends of a GPU child end the run, the
environment a child gets, the result readers and run-at-most-once.  Every child here is a `python -c` one-liner that
imports neither torch nor the library; no GPU process is made to fault."""
import os

import pytest

import gpu_child

TRACEBACK = 'Traceback (most recent call last):\n  File "x.py", line 1, in <module>\nAssertionError: 3 != 4\n'
PRINT_ENV = "import json, os; print(json.dumps(dict(os.environ)))"


@pytest.fixture
def fresh():
    """the runner's remembered fatal end and run_once table, put back after the test whatever its outcome"""
    fatal, once = gpu_child._fatal, dict(gpu_child._once)
    gpu_child._fatal = None
    yield
    gpu_child._fatal = fatal
    gpu_child._once.clear()
    gpu_child._once.update(once)


FATAL = {
    "time limit": dict(returncode=0, timed_out=True, stderr=""),
    **{f"status {rc}": dict(returncode=rc, timed_out=False, stderr="") for rc in (-6, -11, 134, 139, 124, 137)},
    "the child's own HIP status": dict(returncode=2, timed_out=False, stderr="", hip_error_status=2),
    "torch's words": dict(returncode=1, timed_out=False, stderr=TRACEBACK + "RuntimeError: HIP error: an illegal memory access\n"),
    "MVS_ERR_HIP": dict(returncode=1, timed_out=False, stderr=TRACEBACK + "MvsError: libmvs_hip status 4: hipLaunchKernel failed\n"),
}
ORDINARY = {
    "status 0 with the words": dict(returncode=0, timed_out=False, stderr="HIP error\nlibmvs_hip status 4: x\n"),
    "a traceback": dict(returncode=1, timed_out=False, stderr=TRACEBACK),
    "status 2 of another child": dict(returncode=2, timed_out=False, stderr=TRACEBACK),
    "a refusal": dict(returncode=1, timed_out=False, stderr="libmvs_hip status 1: h and w must be positive multiples of 8\n"),
}


@pytest.mark.parametrize("end", list(FATAL))
def test_fatal_ends(end):
    reason = gpu_child.fatal_reason(**FATAL[end])
    assert isinstance(reason, str) and reason


@pytest.mark.parametrize("end", list(ORDINARY))
def test_ordinary_ends(end):
    assert gpu_child.fatal_reason(**ORDINARY[end]) is None


def test_an_aborted_gpu_child_ends_the_run_and_the_next_one_is_not_started(fresh, tmp_path):
    with pytest.raises(pytest.exit.Exception) as e:
        gpu_child.run(["-c", "import sys; print('out'); sys.exit(134)"], env={"MVS_X": "1"}, timeout=60)
    assert e.value.returncode == 3
    assert "status 134" in str(e.value.msg) and "MVS_X" in str(e.value.msg) and "out" in str(e.value.msg)
    mark = tmp_path / "started"
    with pytest.raises(pytest.exit.Exception) as e:
        gpu_child.run(["-c", f"open({str(mark)!r}, 'w').close()"], timeout=60)
    assert e.value.returncode == 3 and "status 134" in str(e.value.msg)
    assert not mark.exists()
    assert gpu_child.run(["-c", "print(7)"], timeout=60, gpu=False).stdout == "7\n"      # host children still run


def test_a_gpu_child_past_its_time_limit_ends_the_run_and_is_gone(fresh, tmp_path):
    pidfile = tmp_path / "pid"
    code = f"import os, time; open({str(pidfile)!r}, 'w').write(str(os.getpid())); print('up', flush=True); time.sleep(60)"
    with pytest.raises(pytest.exit.Exception) as e:
        gpu_child.run(["-c", code], timeout=1)
    assert e.value.returncode == 3 and "time limit" in str(e.value.msg)
    with pytest.raises(ProcessLookupError):
        os.kill(int(pidfile.read_text()), 0)
    assert gpu_child._fatal


def test_nothing_is_fatal_for_a_host_child(fresh):
    r = gpu_child.run(["-c", "import sys; sys.exit(134)"], timeout=60, gpu=False)
    assert r.returncode == 134 and not r.timed_out
    r = gpu_child.run(["-c", "import time; print('up', flush=True); time.sleep(60)"], timeout=1, gpu=False)
    assert r.timed_out and r.returncode != 0 and r.stdout == "up\n" and r.seconds < 30
    assert gpu_child._fatal is None


def test_child_environment(fresh, monkeypatch):
    monkeypatch.setenv("MVS_FOO", "1")
    monkeypatch.setenv("MVS_LIB_PATH", "/x")
    monkeypatch.setenv("RANK", "3")
    for name in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        monkeypatch.delenv(name, raising=False)
    seen = gpu_child.run(["-c", PRINT_ENV], env={"MVS_BAR": "2", "OTHER": "z"}, timeout=60).json()
    assert "MVS_FOO" not in seen and seen["MVS_LIB_PATH"] == "/x" and seen["RANK"] == "3"
    assert seen["MVS_BAR"] == "2" and seen["OTHER"] == "z"
    assert "HIP_VISIBLE_DEVICES" not in seen and "ROCR_VISIBLE_DEVICES" not in seen
    assert seen["PATH"] == os.environ["PATH"]
    seen = gpu_child.run(["-c", PRINT_ENV], timeout=60, gpu=False, drop=("RANK",)).json()
    assert "MVS_FOO" not in seen and seen["MVS_LIB_PATH"] == "/x" and "RANK" not in seen
    assert seen["HIP_VISIBLE_DEVICES"] == "" and seen["ROCR_VISIBLE_DEVICES"] == ""


def test_scripts_are_named_relative_to_the_tests_and_programs_run_as_given(fresh, tmp_path):
    script = tmp_path / "hello.py"
    script.write_text("import sys; print('R ' + sys.argv[1])\n")
    rel = os.path.relpath(script, gpu_child.HERE)
    assert gpu_child.run([rel, 5], timeout=60, gpu=False).records("R ") == [5]
    assert gpu_child.run([script, 6], timeout=60, gpu=False).records("R ") == [6]
    r = gpu_child.run(["/bin/sh", "-c", "echo $0 >&2; exit 5"], timeout=60, gpu=False, python=False)
    assert (r.returncode, r.stdout, r.stderr) == (5, "", "/bin/sh\n")


def test_result_readers():
    out = 'noise\n{"a": 1}\nR {"k": 2}\n {"indented": 0}\nR {"k": 1}\n{"a": 2}\nR2 {"k": 9}\ntail\n'
    r = gpu_child.Child(0, out, "", 0.0)
    assert r.json() == {"a": 2}
    assert r.records("R ") == [{"k": 2}, {"k": 1}]
    assert r.records("R2 ") == [{"k": 9}]


def test_run_once_starts_its_child_once(fresh, tmp_path):
    log = tmp_path / "log"
    code = f"open({str(log)!r}, 'a').write('x'); import sys; sys.exit(1)"
    a = gpu_child.run_once(("host test", 1), ["-c", code], timeout=60, gpu=False)
    b = gpu_child.run_once(("host test", 1), ["-c", code], timeout=60, gpu=False)
    assert a is b and a.returncode == 1 and log.read_text() == "x"       # once, whatever its end
    gpu_child.run_once(("host test", 2), ["-c", code], timeout=60, gpu=False)
    assert log.read_text() == "xx" and a.seconds > 0
