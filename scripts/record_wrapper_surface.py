#!/usr/bin/env python3
"""Records tests/golden/wrapper_surface.json: what tests/wrapper_script.py takes of the Python wrapper -- the names and signatures the classes
expose, every option converter's struct bytes on a fixed list of inputs, and the library calls every method makes on a stand-in library.  Run
it from the commit whose wrapper is to be pinned, BEFORE the wrapper is changed; tests/test_wrapper_surface.py compares against it.  It needs the
built library (for the *_default entry points) and no GPU.
    python scripts/record_wrapper_surface.py <commit the wrapper is recorded from> [output file]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import wrapper_script as S  # noqa: E402


def write(record, path):
    """one entry per line, so that a re-recording reads as a diff of the entries that changed"""
    one = lambda v: json.dumps(v, separators=(", ", ": "))
    parts = [f' "recorded_from": {one(record["recorded_from"])}', f' "excluded": {one(record["excluded"])}']
    for part in ("surface", "options", "traces"):
        groups = []
        for name, entries in record[part].items():
            if isinstance(entries, dict):
                lines = ",\n".join(f"   {one(k)}: {one(v)}" for k, v in entries.items())
                groups.append(f"  {one(name)}: {{\n{lines}\n  }}")
            else:
                groups.append(f"  {one(name)}: {one(entries)}")
        parts.append(f' {one(part)}: {{\n' + ",\n".join(groups) + "\n }")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(parts) + "\n}\n")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "wrapper_surface.json")
    record = S.record(sys.argv[1])
    write(record, out)
    with open(out) as f:
        assert json.load(f) == record
    print(out, {k: len(v) for k, v in record.items() if isinstance(v, dict)})
