"""The Python host around a prediction against tests/golden/host_plumbing.json.gz: what it did on the commit before the blocks
behind the confidences were stated once (score.BLOCKS) - tools/record_host_plumbing.py wrote the file there and explains its
sections.  The recorder runs again here and every row must be the file's: signatures, parsers, the layout grid with passes,
SS and exposure, Outputs over all presence patterns, the exact set_option calls of Engine._call_options, the agreement rules,
the files batch.write_result writes and the summary line of batch.main.  The Flags that Pipeline.submit forms are held through
agree_options, agree_passes and agree_ss only: on the recorded commit they were formed inside `submit`, behind the GPU.
No GPU, no library."""
import gzip
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with gzip.open(os.path.join(ROOT, "tests", "golden", "host_plumbing.json.gz"), "rt") as _fh:
    GOLDEN = json.load(_fh)

_spec = importlib.util.spec_from_file_location("record_host_plumbing", os.path.join(ROOT, "tools", "record_host_plumbing.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)


@pytest.fixture(scope="module")
def live():
    return REC.record()


def test_the_file_is_the_recorders_grid():
    assert set(GOLDEN) == {"signatures", "parsers", "layout", "outputs", "call_options", "agreement", "batch_files", "batch_summary",
                           "texts"}
    assert len(GOLDEN["layout"]) == 2 * 8 * 2 * 3 * 2 * 2 and len(GOLDEN["outputs"]) == 2 ** 9
    assert len(GOLDEN["call_options"]) == 2 * 2 ** 10 and len(GOLDEN["agreement"]) == 32 * 32 + 1 + 24 + 8
    assert [fmt for fmt, _ in GOLDEN["batch_files"]] == ["pdb", "ca", "npz"]
    # (the recorder checks that what raised had set nothing and that what ran left the options as they were)
    assert sum(value[0] == "raised" for _, value in GOLDEN["call_options"]) == 384


@pytest.mark.parametrize("section", ["signatures", "parsers", "layout", "outputs", "call_options", "agreement", "batch_files",
                                     "batch_summary"])
def test_every_row_is_the_recorded_one(live, section):
    texts, live_texts = dict(GOLDEN["texts"]), dict(live["texts"])

    def spelt(value, table):
        """The indices of a call_options / agreement row as the texts they stand for."""
        if section == "call_options":
            return [value[0] if value[0] == "raised" else table[value[0]], table[value[1]]]
        if section == "agreement" and isinstance(value, list) and value[:1] == ["raised"]:
            return ["raised", table[value[1]]]
        return value
    assert [case for case, _ in live[section]] == [case for case, _ in GOLDEN[section]]
    for (case, want), (_, got) in zip(GOLDEN[section], live[section]):
        assert spelt(got, live_texts) == spelt(want, texts), (section, case)
