"""tests/children.py on children that touch no GPU and import nothing of the project: `python -c` on a line or two, statuses from sys.exit(n),
no signal raised.  What an ending means (return, failed test, end of the whole run) is decided here for every child the suite starts."""
import socket
import sys
import time

import pytest

import children


def py(code, *args):
    return [sys.executable, "-c", code] + list(args)


def stops(call, *args, **kw):
    with pytest.raises(pytest.exit.Exception) as e:
        call(*args, **kw)
    assert e.value.returncode == children.STOP_EXIT == 3
    return str(e.value)


def test_result_is_the_last_result_line_and_digests_come_in_order():
    c = children.run(py("print('RESULT [1]'); print('DIGEST a b'); print('noise'); print('RESULT {\"x\": 2}'); print('DIGEST c')"), limit=20)
    assert c.returncode == 0 and c.result() == {"x": 2}
    assert c.digests() == [("a", "b"), ("c",)]


def test_an_ordinary_failure_is_a_failed_test_with_the_stderr_tail():
    with pytest.raises(AssertionError) as e:            # (pytest.exit.Exception is no AssertionError: the run would go on)
        children.run(py("import sys; print('on stdout'); sys.stderr.write('the reason\\n'); sys.exit(1)"), limit=20, env={"PS_X": "7"})
    text = str(e.value)
    assert "the reason" in text and "ended with 1" in text and "PS_X" in text
    assert not issubclass(pytest.exit.Exception, AssertionError)


@pytest.mark.parametrize("status", [124, 134, 137, 139])
def test_a_fault_status_ends_the_run(status):
    text = stops(children.run, py("import sys; sys.stderr.write('last words\\n'); sys.exit(%d)" % status), limit=20)
    assert "ended with %d" % status in text and "last words" in text


def test_the_time_limit_ends_the_run():
    t0 = time.time()
    text = stops(children.run, py("import time; time.sleep(30)"), limit=1)
    assert time.time() - t0 < 2.5
    assert "ended with 124" in text


def test_a_fault_text_ends_the_run_whatever_the_status():
    stops(children.run, py("import sys; sys.stderr.write('HIP error: an illegal memory access was encountered\\n')"), limit=20)
    stops(children.run, py("print('Memory access fault by GPU node-1')"), limit=20)
    children.run(py("print('out of device memory')"), limit=20)        # forced by test_gpu_memory: no fault


def test_expect_names_the_missing_string():
    code = "import sys; print('PS_A=1 is active'); sys.stderr.write('PS_B=0 is active\\n')"
    children.run(py(code), limit=20, expect=("PS_A=1 is active", "PS_B=0 is active"))      # either stream
    with pytest.raises(AssertionError, match="PS_C=1 is active"):
        children.run(py(code), limit=20, expect=("PS_A=1 is active", "PS_C=1 is active"))


def test_drop_and_env(monkeypatch):
    monkeypatch.setenv("PS_LIB", "/somewhere/lib.so")
    code = "import os; print(os.environ.get('PS_LIB')); print(os.environ.get('PS_EXTRA'))"
    assert children.run(py(code), limit=20, drop=("PS_LIB",), env={"PS_EXTRA": "5"}).stdout.split() == ["None", "5"]
    assert children.run(py(code), limit=20).stdout.split() == ["/somewhere/lib.so", "None"]
    assert children.run(py(code), limit=20, drop=("PS_LIB",), env={"PS_LIB": "other"}).stdout.split() == ["other", "None"]   # env after drop


def test_a_group_returns_its_children_in_order():
    group = children.run_group([py("print('RESULT %d')" % r) for r in range(2)], limit=20)
    assert [c.result() for c in group] == [0, 1]


def test_a_fault_in_any_rank_ends_the_run():
    text = stops(children.run_group, [py("import sys; sys.exit(1)"), py("import sys; sys.exit(139)")], limit=20)   # before the 1 is asserted
    assert "ended with 139" in text


def test_a_child_pytest_that_stopped_stops_the_parent():
    stops(children.check_pytest, py("import sys; print('1 passed'); sys.exit(3)"), limit=20)
    with pytest.raises(AssertionError):
        children.check_pytest(py("print('no tests ran')"), limit=20)
    with pytest.raises(AssertionError):
        children.check_pytest(py("print('1 failed, 2 passed')"), limit=20)
    c = children.check_pytest(py("import os; print(os.environ['PS_TEST_CHILD'], os.environ['PS_Y']); print('2 passed in 0.1s')"), limit=20, env={"PS_Y": "y"})
    assert c.stdout.split()[:2] == ["1", "y"]


def test_python_and_script_children_get_their_arguments():
    assert children.script_argv("mp_rank.py", "case", 2)[1:] == [children.HERE + "/mp_rank.py", "case", "2"]
    compile(children.PREAMBLE, "PREAMBLE", "exec")


def test_free_port_base_gives_ports_that_bind():
    base = children.free_port_base(3)
    socks = [socket.socket(socket.AF_INET, socket.SOCK_STREAM) for _ in range(3)]
    try:
        for q, sk in enumerate(socks):
            sk.bind(("127.0.0.1", base + q))
    finally:
        for sk in socks:
            sk.close()
