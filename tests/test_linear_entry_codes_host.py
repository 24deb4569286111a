"""The return code of every dense W4 cdna4 linear entry of the C ABI, case by case, against the table recorded before the entries were moved
onto linear_route (tools/linear_entry_codes.py; tests/linear_entry_codes.json names the commit that produced it): NULL in each position, bad
dtype / group / m / n / k, each misaligned pointer -- bias and sz_half in every row-count class -- alone and in pairs.

Host only: every replayed case is refused by the entry's own argument checks, over fake pointers that are never dereferenced.  The cases
the recording build accepted (null in the table: a misaligned bias on a row count whose kernel reads it by elements, a misaligned sz_half
that takes the sz_packed path) would reach a launch and are not replayed.
"""
import json

import pytest

from tools import linear_entry_codes as lc

with open(lc.TABLE) as _f:
    _TABLE = json.load(_f)


def test_table_covers_the_six_entries():
    assert sorted(_TABLE["entries"]) == sorted(lc.ENTRIES) and len(lc.ENTRIES) == 6
    assert len(_TABLE["generated_from"]) == 40


@pytest.mark.parametrize("entry", lc.ENTRIES)
def test_entry_codes_match_the_recorded_table(entry):
    from llm_awq_amd import _capi

    want, cases = _TABLE["entries"][entry], lc.cases(entry)
    assert lc.ids_digest(cases) == want["ids"] and len(cases) == len(want["codes"]), "the case generator has drifted from the table"
    fn = getattr(_capi.lib(), entry)
    replayed = [(cid, fn(*args.values()), code) for (cid, args), code in zip(cases, want["codes"]) if code is not None]
    assert len(replayed) > 500
    wrong = [(cid, got, code) for cid, got, code in replayed if got != code]
    assert not wrong, f"{len(wrong)} of {len(replayed)} cases changed their code (id, now, recorded): {wrong[:10]}"
