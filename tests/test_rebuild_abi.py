"""CPU-side checks of srtRebuildScene and srtGetTreeCost (no GPU): the ctypes prototypes of hipdev.py against
include/srt_hip.h, the export table, the binding's methods, the host layer and the example compiling against the
declarations, and the entries' behaviour without a context."""
import ctypes as C
import inspect
import os
import subprocess

from conftest import ROOT
import abi_header

ENTRIES = ("srtRebuildScene", "srtGetTreeCost")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "g++"


def test_ctypes_prototypes_match_header(dev, abi):
    decls = abi_header.declarations("srt_hip.h")
    for name in ENTRIES:
        assert name in decls and name in dev.EXPORTS and name not in dev.TEST_EXPORTS
        assert hasattr(dev.lib, name)
        assert getattr(dev.lib, name).restype is C.c_int and decls[name][0] == "int"
        abi_header.assert_prototype(dev, abi, name)
    assert decls["srtRebuildScene"][1] == decls["srtRefitScene"][1] == ["SrtContext*", "void*"]
    # (abi_header's table has no double: the interface's one double* is an address, c_void_p, which byref() satisfies)
    assert decls["srtGetTreeCost"][1] == ["SrtContext*", "int32_t", "double*"]
    assert dev.lib.srtGetTreeCost.argtypes == [C.c_void_p, C.c_int32, C.c_void_p]


def test_binding_methods(dev):
    par = inspect.signature(dev.Context.rebuild).parameters
    assert list(par) == ["self", "stream"] and par["stream"].default is None
    par = inspect.signature(dev.Context.tree_cost).parameters
    assert list(par) == ["self", "item"] and par["item"].default == 0


def test_entries_fail_without_a_context(dev):
    cost = C.c_double(7.5)
    assert dev.lib.srtRebuildScene(None, None) != 0
    assert dev.lib.srtGetTreeCost(None, 0, C.byref(cost)) != 0
    assert dev.lib.srtGetTreeCost(None, 0, None) != 0
    assert cost.value == 7.5


def test_host_layer_and_example_compile_with_the_new_calls(tmp_path, dev):
    host = os.path.join(ROOT, "sexy-raytracer_amd", "host")
    subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    main = open(os.path.join(ROOT, "examples", "main.cpp")).read()
    assert all(s in main for s in ('"--tree-cost"', "treeCost("))
    src = tmp_path / "rebuild_call.cpp"
    src.write_text("""
#include "srt/device.h"
#include <type_traits>
static_assert(std::is_same<decltype(&srtRebuildScene), int (*)(SrtContext*, void*)>::value, "rebuild");
static_assert(std::is_same<decltype(&srtGetTreeCost), int (*)(SrtContext*, int32_t, double*)>::value, "cost");
bool frame(hipDevice& d, double& before, double& after) {
  return d.treeCost(0, before) && d.updateTriangles(0, d.triangles) && d.rebuild() && d.treeCost(0, after) && d.refit();
}
""")
    subprocess.check_call([HIPCC, "-std=c++17", "-fsyntax-only", "-Wall", "-I" + host, "-I" + os.path.join(ROOT, "include"),
                           "-x", "c++", str(src)])
