"""The one runner for the child processes the suite starts: forced storage forms, poison runs, the release library, rank processes, child
pytest runs and bench.py.  Switches are read once per process, so every alternative path needs a process of its own, and every such process
goes through run() below, which decides in ONE place what the child's ending means:

  * a status below 0, one of FAULT_STATUSES (the time limit of `timeout`, an abort, a kill, a segmentation fault) or one of FAULT_TEXTS in
    either stream ends the WHOLE pytest run with status STOP_EXIT: nothing more is started on a GPU that has just faulted or hung;
  * any other non-zero status is an AssertionError with the tail of the output, an ordinary failed test;
  * status 0 returns a Child, after every string of `expect` has been found in its output.

Every child runs under `timeout -k 10 LIMIT`, which puts it into a process group of its own and signals the group: the rank processes or the
children of a child pytest end with it.  The in-process case is not covered: a PolyStokesError whose text reports an illegal access inside the
pytest process itself still fails only its test (stopping there takes a hook in conftest.py).  Plain functions, no fixtures."""
import json
import os
import signal
import socket
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

STOP_EXIT = 3                               # the status of a pytest run that a child's fault or time limit ended
FAULT_STATUSES = (124, 134, 137, 139)       # timeout(1): the limit ran out / 128 + SIGABRT / 128 + SIGKILL (after -k) / 128 + SIGSEGV
# hipErrorIllegalAddress as hipGetErrorString words it (ps_last_error and torch carry it) / the ROCr runtime's line on stderr before it aborts
# the process on a page fault of the GPU / hipErrorLaunchFailure.  Nothing else: out-of-memory texts are forced by test_gpu_memory.
FAULT_TEXTS = ("an illegal memory access was encountered", "Memory access fault", "unspecified launch failure")

IS_CHILD_RUN = os.environ.get("PS_TEST_CHILD") == "1"      # this pytest IS the child of run_pytest()

# the first lines of every inline program (run_python)
PREAMBLE = ("import json, os, sys\n"
            f"sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {HERE!r})\n"
            "import numpy as np\n"
            "import polystokes_amd\n"
            "from polystokes_amd import scenes, _abi as abi\n")


class Child:
    def __init__(self, argv, env, returncode, stdout, stderr):
        self.argv, self.env, self.returncode, self.stdout, self.stderr = argv, env, returncode, stdout, stderr

    @property
    def output(self):
        """both streams, for messages and for texts either of them may carry"""
        return self.stdout + ("\n" if self.stdout and not self.stdout.endswith("\n") else "") + self.stderr

    def describe(self):
        argv = " ".join(a if len(a) <= 200 else a[:200] + "..." for a in self.argv)
        return "child %s (env %r) ended with %d: %s" % (argv, self.env, self.returncode, self.output[-2000:])

    def result(self):
        """the JSON of the last stdout line 'RESULT <json>'"""
        return json.loads([ln for ln in self.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])

    def digests(self):
        """the tokens after DIGEST of every such stdout line, in order"""
        return [tuple(ln.split()[1:]) for ln in self.stdout.splitlines() if ln.startswith("DIGEST ")]


def _start(argv, limit, env, drop):
    full = {k: v for k, v in os.environ.items() if k not in drop}
    full.update(env or {})
    return subprocess.Popen(["timeout", "-k", "10", str(limit)] + list(argv), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=full)


def _collect(proc, argv, limit, env):
    try:
        out, err = proc.communicate(timeout=limit + 30)
    except subprocess.TimeoutExpired:      # the backstop: `timeout` itself did not end (its group id is its pid)
        try:
            os.killpg(proc.pid, signal.SIGKILL)
        except OSError:
            proc.kill()
        out, err = proc.communicate()
    return Child(list(argv), dict(env or {}), proc.returncode, out, err)


def _stop_on_fault(child, stop=()):
    rc = child.returncode
    if rc < 0 or rc in FAULT_STATUSES or rc in stop or any(t in child.output for t in FAULT_TEXTS):
        pytest.exit(child.describe(), returncode=STOP_EXIT)


def _check(child, expect):
    assert child.returncode == 0, child.describe()
    for text in expect:
        assert text in child.output, "%r is not in the output: %s" % (text, child.describe())
    return child


def run(argv, *, limit, env=None, drop=(), expect=(), stop=()):
    """argv under `timeout -k 10 limit`, with os.environ minus `drop` plus `env`; `stop`: further statuses that end the run"""
    child = _collect(_start(argv, limit, env, drop), argv, limit, env)
    _stop_on_fault(child, stop)
    return _check(child, expect)


def run_group(argvs, *, limit, env=None, drop=(), expect=()):
    """rank processes: all started, each under its own limit, all collected, and every ending classified before anything is asserted"""
    procs = [_start(argv, limit, env, drop) for argv in argvs]
    group = [_collect(proc, argv, limit, env) for proc, argv in zip(procs, argvs)]
    for child in group:
        _stop_on_fault(child)
    return [_check(child, expect) for child in group]


def run_python(code, *args, **kw):
    return run([sys.executable, "-c", PREAMBLE + code] + [str(a) for a in args], **kw)


def script_argv(name, *args):
    """a file under tests/: the *_cases.py mains, mp_rank.py, affine_child.py"""
    return [sys.executable, os.path.join(HERE, name)] + [str(a) for a in args]


def run_script(name, *args, **kw):
    return run(script_argv(name, *args), **kw)


def check_pytest(argv, *, env=None, **kw):
    """a child pytest: a status of STOP_EXIT means its own runner has stopped it on a fault, so this run stops too"""
    child = run(argv, env=dict(env or {}, PS_TEST_CHILD="1"), stop=(STOP_EXIT,), **kw)
    assert " passed" in child.output and "failed" not in child.output, child.describe()
    return child


def run_pytest(path, k, **kw):
    return check_pytest([sys.executable, "-m", "pytest", os.path.abspath(path), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "-k", k], **kw)


def free_port_base(n):
    """a base port with n consecutive free ports (checked by binding them once)"""
    for base in range(30100 + (os.getpid() % 500) * 8, 40000, 64):
        socks = []
        try:
            for q in range(n):
                sk = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
                sk.bind(("127.0.0.1", base + q))
                socks.append(sk)
            return base
        except OSError:
            continue
        finally:
            for sk in socks:
                sk.close()
    raise RuntimeError("no free port range")
