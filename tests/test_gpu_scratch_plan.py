"""The built library holds the scratch and runs the stream chunks it did when tests/golden/scratch_plan_parent.json was recorded
(tools/scratch_table.py on an MI355X, before the sizing moved into airwave_amd/csrc/host/scratch_plan.hpp): for every row the pool's bytes
after the reserve and after each call, the launch counts of the partitioned and the long-window kernels and info()'s long-window rows —
and the host entry's streams per staged chunk.  A row that either side lacks is a failure.  tests/test_scratch_plan_host.py replays the
same file on the CPU."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("_scratch_table_under_test", os.path.join(ROOT, "tools", "scratch_table.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_rows_are_the_recorded_ones(tool, golden_dir):
    text = open(os.path.join(golden_dir, "scratch_plan_parent.json")).read()
    want = json.loads(text)
    header, results = tool.run_all()
    assert header == want["header"]
    assert [r["name"] for r in results] == [r["name"] for r in want["rows"]]
    different = [(got, rec) for got, rec in zip(results, want["rows"]) if got != rec]
    assert not different, different
    assert tool.dumps(header, results) == text          # byte for byte what the tool wrote
