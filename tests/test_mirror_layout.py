"""The layout of the Python mirror ("layout of the Python mirror"): rotation_representation is the facade over the family
modules, every module stands on _runtime and imports on its own, the runtime's state exists once, and the optional-helper notices are
printed once per process.  No GPU, and no library: importing the package must not load it."""
import glob
import os
import subprocess
import sys

import pytest

import poseestimation_amd as pa
from poseestimation_amd import _runtime, rotation_representation as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(ROOT, "poseestimation_amd", "*.py")) if not p.endswith("__init__.py"))
FAMILIES = ("symmetry", "angle_statistics", "clouds", "neighbors", "pointnet", "pose_losses")


def child(code):
    flags = ["-s"] if sys.flags.no_user_site else []
    return subprocess.run([sys.executable, *flags, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)


def test_the_module_list_is_the_one_this_file_knows():
    assert set(FAMILIES) | {"_runtime", "rotation_representation", "_lib", "build", "distributed"} == set(MODULES)


def test_every_public_name_is_the_same_object_on_the_facade():
    assert len(set(pa.__all__)) == len(pa.__all__)
    for name in pa.__all__:
        assert getattr(pa, name) is getattr(rr, name), name


def test_the_facade_hands_out_each_family_s_own_objects():
    import importlib
    for family in FAMILIES:
        module = importlib.import_module("poseestimation_amd." + family)
        own = [n for n, o in vars(module).items() if not n.startswith("_") and getattr(o, "__module__", None) == module.__name__]
        assert own, family
        for name in own:
            assert getattr(rr, name) is getattr(module, name), (family, name)


@pytest.mark.parametrize("module", MODULES)
def test_each_module_imports_alone_without_loading_the_library(module):
    out = child("import poseestimation_amd.%s as m, poseestimation_amd._lib as l, sys\n"
                "assert l._lib is None, 'the import loaded libso3proj.so'\n"
                "assert 'poseestimation_amd._runtime' in sys.modules\n" % module)
    assert out.returncode == 0, out.stderr


def test_imports_form_a_tree_under_the_runtime():
    """Read from the sources: a family imports _lib, _runtime and the families the design allows it, never the facade; the runtime's
    functions are bound by name (`from ._runtime import ...`), never reached through a module attribute."""
    import ast
    allowed = {"_runtime": {"_lib"}, "neighbors": {"_lib", "_runtime", "pointnet"}, "pose_losses": {"_lib", "_runtime", "symmetry"}}
    for module in FAMILIES + ("_runtime", "rotation_representation"):
        tree = ast.parse(open(os.path.join(ROOT, "poseestimation_amd", module + ".py")).read())
        siblings = set()
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level == 1:
                assert node.module or "_runtime" not in {a.name for a in node.names}, module       # no `from . import _runtime`
                siblings |= {node.module} if node.module else {a.name for a in node.names}
            elif isinstance(node, ast.Import):
                assert not any(a.name.startswith("poseestimation_amd") for a in node.names), module
            elif isinstance(node, ast.ImportFrom):
                assert node.level == 0 and not (node.module or "").startswith("poseestimation_amd"), module
        if module == "rotation_representation":
            assert siblings == set(FAMILIES) | {"_lib", "_runtime"}
        else:
            assert siblings <= allowed.get(module, {"_lib", "_runtime"}), (module, siblings)


def test_the_runtime_state_exists_once():
    for name in ("_WARNED", "_ZERO_POOL", "_STAT_WORKSPACES"):
        assert getattr(rr, name) is getattr(_runtime, name), name
    import importlib
    for module in ("rotation_representation",) + FAMILIES:
        m = importlib.import_module("poseestimation_amd." + module)
        for name in ("_WARNED", "_ZERO_POOL", "_STAT_WORKSPACES", "_WORKSPACES", "_FAST", "_ROW_HEADS"):
            assert getattr(m, name, getattr(_runtime, name)) is getattr(_runtime, name), (module, name)
        for name in ("_L", "_NODE_BOUND", "_DEVICE_COUNT"):                      # rebound inside _runtime: never copied out of it
            assert not hasattr(m, name), (module, name)
    assert rr._workspace.__globals__["_WORKSPACES"] is _runtime._WORKSPACES


def test_a_missing_helper_is_announced_once_per_process():
    """With both optional helpers made unimportable, a process that imports the whole package, module by module, prints each notice
    exactly once (at _runtime's import)."""
    out = child("import sys\n"
                "sys.modules['poseestimation_amd._so3fast'] = sys.modules['poseestimation_amd._so3node'] = None\n"
                "import poseestimation_amd\n" + "".join("import poseestimation_amd.%s\n" % m for m in MODULES) +
                "from poseestimation_amd import _runtime\n"
                "assert _runtime._so3fast is None and _runtime._so3node is None\n")
    assert out.returncode == 0, out.stderr
    for helper in ("_so3fast", "_so3node"):
        assert out.stderr.count("[poseestimation_amd] optional helper %s is not available" % helper) == 1, out.stderr
