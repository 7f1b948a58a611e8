"""INTEGRATION.md §2 shows the C# (P/Invoke) binding a maintainer would add; no .NET SDK exists in this image, so it cannot be compiled.
What CAN be held: that the text is a binding of THIS header -- every [DllImport] names a function include/ocean_waves.h declares, with the
same number of arguments and a return type of the same width, and every [StructLayout] struct lists the fields of its C struct in the same
order with types of the same size (so that LayoutKind.Sequential reproduces the C layout) -- and that §7's index names every export."""
import re
from checks import c_functions, c_struct_fields, cs_struct_fields, DOC, SHIM, strip_comments


STRUCTS = {"OwCascadeParams": "ow_cascade_params", "OwConfig": "ow_config", "OwSurfaceSample": "ow_surface_sample", "OwGroupLink": "ow_group_link",
           "OwGroupConfig": "ow_group_config"}


def test_every_dllimport_is_a_function_of_the_header_with_the_same_shape():
    cfun = c_functions()
    imports = re.findall(r"\[DllImport\(Lib\)\]\s*public static extern (\w+) (ow_[a-z0-9_]+)\((.*?)\);", strip_comments(SHIM))
    assert len(imports) >= 30
    for ret, name, args in imports:
        assert name in cfun, f"{name}: not declared in include/ocean_waves.h"
        c_ret, c_n = cfun[name]
        n = 0 if not args.strip() else args.count(",") + 1
        assert n == c_n, f"{name}: {n} arguments in the shim, {c_n} in the header"
        width = {"void": 0, "int": 4, "IntPtr": 8, "double": 8}[ret]
        c_width = 0 if c_ret == "void" else (8 if c_ret.endswith("*") or c_ret == "double" else 4)
        assert width == c_width, f"{name}: returns {ret} in the shim, {c_ret} in the header"
    # the calls the reference's own scene code maps to are all bound
    for must in ("ow_create", "ow_destroy", "ow_update", "ow_process", "ow_cascades_remaining", "ow_set_cascade_params", "ow_get_device_ptrs",
                 "ow_readback_begin", "ow_readback_wait", "ow_last_error"):
        assert must in [i[1] for i in imports], must


def test_every_shim_struct_lists_the_fields_of_its_c_struct():
    for cs, c in STRUCTS.items():
        want, got = c_struct_fields(c), cs_struct_fields(cs)
        assert [f for f, _ in got] == [f for f, _ in want], f"{cs}: fields {got} against {c}: {want}"
        assert [s for _, s in got] == [s for _, s in want], f"{cs}: field sizes {got} against {c}: {want}"
    assert sum(s for _, s in c_struct_fields("ow_cascade_params")) == 128   # no padding: every double sits on a multiple of 8
    assert sum(s for _, s in c_struct_fields("ow_surface_sample")) == 64
    assert sum(s for _, s in c_struct_fields("ow_group_link")) == 32


def test_the_index_names_every_export():
    index = DOC.split("## 7. Index")[1]
    missing = [name for name in c_functions() if "`%s`" % name not in index]
    assert not missing, missing
    assert "(%d;" % len(c_functions()) in index.splitlines()[0]
