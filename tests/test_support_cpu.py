"""The rule of the test support: helpers live in tests/support.py (no device), tests/gpu_support.py (device), tests/refusals.py (the library's
refusals before any launch) and the *_scenes.py modules, and no test module is another one's library."""
import ast
import glob
import os


def test_no_test_imports_another_and_the_host_side_helpers_stay_host_side():
    here = os.path.dirname(os.path.abspath(__file__))
    for path in sorted(glob.glob(os.path.join(here, "*.py"))):
        name, mods = os.path.basename(path), set()
        with open(path) as f:
            for node in ast.walk(ast.parse(f.read())):  # (every import, those inside functions too)
                if isinstance(node, ast.Import):
                    mods |= {a.name for a in node.names}
                elif isinstance(node, ast.ImportFrom):
                    base = ".".join(filter(None, ["tests" if node.level else "", node.module]))
                    mods |= {base} | {f"{base}.{a.name}" for a in node.names}  # (a name imported from the package may be a module)
        assert not [m for m in mods if m.startswith("tests.test_")], (name, sorted(mods))
        host_side = name in ("corner_scenes.py", "support.py")
        if host_side or name.endswith("_cpu.py"):
            assert not [m for m in mods if m.startswith("tests.gpu_support")], (name, sorted(mods))
        if host_side:
            assert not [m for m in mods if m.split(".")[0] == "torch" or m.startswith("fireflies_amd._lib")], (name, sorted(mods))
