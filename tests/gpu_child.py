"""The one place where the suite starts child processes.

Kernel selection is read once per process, so every test of a non-default kernel form runs its check in a child, and
the host tests run the library's refusals in children that see no device.  Each child has its caller's time limit and
is never retried.  After a GPU child that died from a signal, ran into its time limit or met a HIP error the run ends
(pytest.exit, status 3), so that nothing more is started on the GPU: the card may be in the state the child left it in,
and a next child on it can take the machine down.  The reason is remembered, so that a later GPU child is not started
either should something have caught the exit.  A host child (gpu=False) has no fatal end: the caller gets it back and
asserts on it.

Imports no torch and does not touch the GPU itself.
"""
import dataclasses
import json
import os
import subprocess
import sys
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FATAL_STATUS = (134, 139, 124, 137)     # abort, segmentation fault, and the two ends of a `timeout` around the child
HIP_ERROR_TEXTS = ("HIP error", "libmvs_hip status 4:")     # torch's wording; _lib.MvsError of MVS_ERR_HIP
_fatal = None       # the reason of the fatal end this process has seen
_once = {}          # run_once: key -> Child


@dataclasses.dataclass
class Child:
    returncode: int         # -9 after a time limit: the child was killed
    stdout: str
    stderr: str
    seconds: float
    timed_out: bool = False

    def json(self):
        """the last stdout line that starts with "{", parsed"""
        return json.loads([ln for ln in self.stdout.splitlines() if ln.startswith("{")][-1])

    def records(self, prefix):
        return [json.loads(ln[len(prefix):]) for ln in self.stdout.splitlines() if ln.startswith(prefix)]


def fatal_reason(returncode, timed_out, stderr, hip_error_status=None):
    """Why nothing more may run on the GPU after a child with this end, or None."""
    if timed_out:
        return "did not end within its time limit"
    if returncode < 0 or returncode in FATAL_STATUS:
        return f"died with status {returncode}"
    if returncode != 0 and (returncode == hip_error_status or any(t in stderr for t in HIP_ERROR_TEXTS)):
        return f"met a HIP error (status {returncode})"
    return None


def child_env(env=None, gpu=True, drop=()):
    """The parent's environment without its MVS_* switches (MVS_LIB_PATH stays) and the names in `drop`, plus `env`."""
    out = {k: v for k, v in os.environ.items() if (not k.startswith("MVS_") or k == "MVS_LIB_PATH") and k not in drop}
    out.update(env or {})
    if not gpu:
        out.update(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    return out


def _text(s):
    return s if isinstance(s, str) else (s or b"").decode("utf-8", "replace")


def run(argv, *, env=None, timeout, gpu=True, python=True, drop=(), hip_error_status=None):
    """Runs `argv` to its end and returns the Child.  python=True: [sys.executable, *argv], where argv starts with "-c"
    or with a script's name relative to tests/.  python=False: argv as given."""
    global _fatal
    argv = [str(a) for a in argv]
    what = f"{' '.join(a if len(a) < 200 else a[:60] + '...' for a in argv)} {env or {}}"
    if gpu and _fatal:
        pytest.exit(f"{what} not started: an earlier GPU child {_fatal}", returncode=3)
    if python:
        argv = [sys.executable] + (argv if argv[0] == "-c" else [os.path.join(HERE, argv[0])] + argv[1:])
    t0 = time.perf_counter()
    try:
        r = subprocess.run(argv, env=child_env(env, gpu, drop), capture_output=True, text=True, timeout=timeout)
        child = Child(r.returncode, r.stdout, r.stderr, time.perf_counter() - t0)
    except subprocess.TimeoutExpired as e:      # subprocess.run has killed the child and waited for it
        child = Child(-9, _text(e.stdout), _text(e.stderr), time.perf_counter() - t0, timed_out=True)
    print(child.stdout[-8000:])
    print(child.stderr[-3000:])
    print(f"[child] {what}: {child.seconds:.1f} s of {timeout} s, status {child.returncode}")
    reason = gpu and fatal_reason(child.returncode, child.timed_out, child.stderr, hip_error_status)
    if reason:      # no further GPU work in this run
        _fatal = f"{reason}: {what}"
        pytest.exit(f"{what} {reason}:\n{child.stdout[-4000:]}\n{child.stderr[-4000:]}", returncode=3)
    return child


def run_once(key, argv, **kwargs):
    """run(), at most once per key in this process whatever the child's end: later calls get the same Child."""
    if key not in _once:
        _once[key] = run(argv, **kwargs)
    return _once[key]
