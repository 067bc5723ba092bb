"""tests/check.h and tests/hostcheck.py themselves: the one CHECK macro carries the assertions of every *_check.cpp program, so a
failing CHECK must fail the program, name its expression and line, withhold the ok line, and fail the test that runs it."""
import subprocess

import pytest

import hostcheck

PROGRAM = """#include "check.h"
int main() {
    CHECK(1 + 1 == 2);
    CHECK(2 + 2 == %d, "two and two make %%d", 2 + 2);
    return check_finish("tiny ok");
}
"""


def _tiny(tmp_path, four):
    src = tmp_path / f"tiny_{four}.cpp"
    src.write_text(PROGRAM % four)
    return hostcheck.build(tmp_path, f"tiny_{four}", [], src, rocm=False)


def test_a_failing_check_fails_the_test(tmp_path):
    exe = _tiny(tmp_path, 5)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0
    assert "tiny_5.cpp:4" in p.stderr and "2 + 2 == 5" in p.stderr and "two and two make 4" in p.stderr, p.stderr
    assert "1 + 1 == 2" not in p.stdout + p.stderr
    assert "tiny ok" not in p.stdout + p.stderr
    with pytest.raises(AssertionError, match="2 \\+ 2 == 5"):
        hostcheck.run(exe, ok="tiny ok")


def test_passing_checks_print_the_ok_line(tmp_path):
    assert "tiny ok" in hostcheck.run(_tiny(tmp_path, 4), ok="tiny ok")
