"""Every entry point of include/audiocodec_amd.h that takes a stream has a row in the table of test_stream_contract.py, or an
entry in its EXEMPT dict with a reason: a new entry point without either fails here, by name, without a GPU."""

import os
import re

from conftest import ROOT
import test_stream_contract as contract


def _stream_entry_points():
    with open(os.path.join(ROOT, "include", "audiocodec_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    decls = re.findall(r"\bAC_API\s+[^;{}]*?\b(ac_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert "ac_version" in [name for name, _ in decls], "the header's declarations were not found"
    return [name for name, args in decls if re.search(r"\bvoid\s*\*\s*stream\b", args)]


def test_every_stream_taking_entry_point_has_a_row():
    names = _stream_entry_points()
    assert len(names) == len(set(names)) and len(names) >= 43, names
    covered = {c for r in contract.ROWS.values() for c in r.covers}
    missing = [n for n in names if n not in covered and n not in contract.EXEMPT]
    assert not missing, "entry points that take a stream and have no row in test_stream_contract.py: %s" % missing
    # the table names nothing the header does not declare with a stream, and an exemption states its reason
    unknown = sorted((covered | set(contract.EXEMPT)) - set(names))
    assert not unknown, "rows name entry points the header does not declare with a stream: %s" % unknown
    for name, reason in contract.EXEMPT.items():
        assert name not in covered, "%s is exempt and has a row" % name
        assert isinstance(reason, str) and len(reason) >= 20, name


def test_rows_are_well_formed():
    for rid, r in contract.ROWS.items():
        assert r.covers and set(r.checks) <= {"producer", "busy"} and r.checks, rid
        assert callable(r.build), rid
