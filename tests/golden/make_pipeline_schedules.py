"""Record tests/golden/pipeline_schedules.json: for every case of tests/pipeline_cases.py the schedule the
pipeline drivers issue (every library call with its normalised arguments, every stream edge, the kept-zeros flag:
pipeline_cases.Recorder) and the SHA-256 of every output, from the built library and the package's Python on an
MI355X.

The table is self-referential ("pinned_to"): it pins pipeline.py, shpl_map.py and _lib.py across a refactor --
record it from the commit before the change, and tests/test_gpu_pipeline_schedules.py holds every later commit to
it. Nothing in a row depends on an address, a handle or an allocation, so two recordings in separate processes
must be byte-identical.

Log entries repeat across cases, so the file holds each distinct entry once ("entries") and a case's log as
indices into that list.

The raw-scan cases take the `kitti_dir` fixture of tests/conftest.py, so the recording runs as a pytest session
over this file (which the suite never collects: its name is no test file's).

Run (after building the library):  python tests/golden/make_pipeline_schedules.py [OUT.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT_ENV = "PIPELINE_SCHEDULES_OUT"


def test_record(kitti_dir):
    import pipeline_cases as pc
    rows = {name: pc.record_case(name, kitti_dir) for name in pc.CASES}
    entries, index = [], {}
    for row in rows.values():
        packed = []
        for e in row["log"]:
            key = json.dumps(e, sort_keys=True)
            if key not in index:
                index[key] = len(entries)
                entries.append(key)
            packed.append(index[key])
        row["log"] = packed
    out = os.environ.get(OUT_ENV) or pc.TABLE
    with open(out, "w") as fh:
        fh.write('{\n"pinned_to": "self: the commit that recorded it (tests/golden/make_pipeline_schedules.py)",\n')
        fh.write('"entries": [\n%s\n],\n"cases": {\n' % ",\n".join(entries))
        fh.write(",\n".join('"%s": %s' % (k, json.dumps(v, sort_keys=True)) for k, v in rows.items()))
        fh.write("\n}\n}\n")
    print(len(rows), "cases,", len(entries), "distinct entries ->", out)


if __name__ == "__main__":
    import pytest
    if len(sys.argv) > 1:
        os.environ[OUT_ENV] = os.path.abspath(sys.argv[1])
    sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
    sys.exit(pytest.main([os.path.abspath(__file__) + "::test_record", "-q", "-s", "-p", "no:cacheprovider"]))
