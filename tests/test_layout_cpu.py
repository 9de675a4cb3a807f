"""CPU: the layout of tests/ — a test module imports helper modules, never another test module (pytest would hold two copies of it:
the collected `test_x` and the imported `tests.test_x`), and a helper module holds no test."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPORTS_A_TEST_MODULE = re.compile(r"from tests[.]test_|from tests +import test_|import tests[.]test_")          # (no line of this file matches)


def sources():
    for folder in ("tests", "tools"):
        for name in sorted(os.listdir(os.path.join(ROOT, folder))):
            if name.endswith(".py"):
                with open(os.path.join(ROOT, folder, name)) as f:
                    yield folder, name, f.read().split("\n")


def test_no_module_imports_a_test_module_and_no_helper_holds_a_test():
    seen = 0
    for folder, name, lines in sources():
        seen += 1
        bad = [line for line in lines if IMPORTS_A_TEST_MODULE.search(line)]
        assert not bad, f"{folder}/{name} imports a test module: {bad}"
        if folder == "tests" and not name.startswith("test_") and name != "conftest.py":
            bad = [line for line in lines if re.match(r"\s*def test_", line)]
            assert not bad, f"tests/{name} is a helper module and defines a test: {bad}"
    assert seen > 80
