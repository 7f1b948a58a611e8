"""Where the suite's shared scaffolding lives: test modules import the support modules (tests/scenes.py, tests/cpu_builds.py,
tests/checks.py, tests/helpers.py, tests/device_maps.py, tests/raster_soups.py, tests/foam_exact.py, the twins), never one another, and so do the programs under scripts/; and a compiler is started from the
support modules only, apart from the few test modules whose builds are their subject."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the modules that build something no other module builds: the ABI header checks, and the second build of four harnesses under the
# undefined-behaviour sanitizer
OWN_BUILDS = {"test_abi.py", "test_consumer_edges.py"}
SUPPORT_BUILDS = {"cpu_builds.py"}


def test_no_module_imports_a_test_module_and_compilers_start_from_the_support_modules():
    sources = [p for pattern in ("tests/*.py", "tests/golden/*.py", "scripts/*.py") for p in glob.glob(os.path.join(ROOT, pattern))]
    assert sources
    compiles = set()
    for path in sources:
        tree = ast.parse(open(path).read(), path)
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                imported = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                imported = [node.module or ""]
            else:
                imported = []
            assert not any(m.split(".")[-1].startswith("test_") for m in imported), (path, node.lineno, imported)
            if isinstance(node, ast.Constant) and isinstance(node.value, str):    # a child process's script kept in a string
                assert not re.search(r"^\s*(from|import) test_", node.value, flags=re.M), (path, node.lineno)
            # a command line, in a call or kept in a constant: a list that begins with the compiler's name
            if isinstance(node, ast.List) and node.elts and isinstance(node.elts[0], ast.Constant) and node.elts[0].value in ("gcc", "g++", "cc", "c++"):
                compiles.add(os.path.relpath(path, ROOT))
    in_tests = {os.path.basename(p) for p in compiles if os.path.dirname(p) == "tests"}
    assert SUPPORT_BUILDS <= in_tests
    assert in_tests <= SUPPORT_BUILDS | OWN_BUILDS, sorted(in_tests - SUPPORT_BUILDS - OWN_BUILDS)
