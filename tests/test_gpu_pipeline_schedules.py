"""The pipeline drivers (pipeline.py's FusedPipeline and FramePipeline, shpl_map.py's ShplMap, pull and
build_index_batch) held to the schedule recorded in tests/golden/pipeline_schedules.json: every library call with
its arguments, every stream edge, the kept-zeros flag, and the SHA-256 of every output (tests/pipeline_cases.py;
recorded by tests/golden/make_pipeline_schedules.py from the commit before the drivers' clean-up). Output bits
cannot see a lost stream edge; the log can.

Each case runs without timing events and, where its steps take `events`, with them: the events must add their
`record`s at the recorded places and nothing else. Inside the case runner the synthetic 32 + 32 cases are also
held to test_gpu_keep_zeros.py's oracle result of their frames, and the raw-scan cases to test_gpu_parity.py's
oracle chain over the two KITTI frames."""
import functools
import json

import pytest

import pipeline_cases as pc


@functools.lru_cache(maxsize=None)
def _table():
    with open(pc.TABLE) as fh:
        return json.load(fh)


def test_table_covers_the_cases():
    t = _table()
    assert list(t["cases"]) == list(pc.CASES)
    assert not [k for k, v in t["cases"].items() if "unstable" in v]
    for name, row in t["cases"].items():
        assert ("events" in row) == pc.takes_events(name), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(pc.CASES))
def test_schedule_and_bits(name, kitti_dir):
    t = _table()
    want = t["cases"][name]
    got = pc.record_case(name, kitti_dir)
    log = json.loads(json.dumps(got["log"]))  # (tuples and lists alike, as the table holds them)
    assert log == [t["entries"][i] for i in want["log"]]
    assert got["digests"] == want["digests"]
    assert json.loads(json.dumps(got.get("events"))) == want.get("events")
