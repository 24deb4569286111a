"""The return code of every natural-KV-cache entry of the C ABI, case by case, against the table recorded before the entries were folded
onto one descriptor and one check (tools/kv_entry_codes.py; tests/kv_entry_codes.json names the commit that produced it).

Host only: every replayed case is refused by the entry's own argument checks, over fake pointers that are never dereferenced.  The cases
the recording build accepted (null in the table) would reach a launch and are not replayed.
"""
import json

import pytest

from tools import kv_entry_codes as kc

with open(kc.TABLE) as _f:
    _TABLE = json.load(_f)


def test_table_covers_the_twelve_entries():
    assert sorted(_TABLE["entries"]) == sorted(kc.ENTRIES) and len(kc.ENTRIES) == 12
    assert len(_TABLE["generated_from"]) == 40


@pytest.mark.parametrize("entry", kc.ENTRIES)
def test_entry_codes_match_the_recorded_table(entry):
    from llm_awq_amd import _capi

    want, cases = _TABLE["entries"][entry], kc.cases(entry)
    assert kc.ids_digest(cases) == want["ids"] and len(cases) == len(want["codes"]), "the case generator has drifted from the table"
    fn = getattr(_capi.lib(), entry)
    replayed = [(cid, fn(*args.values()), code) for (cid, args), code in zip(cases, want["codes"]) if code is not None]
    assert len(replayed) > 500
    wrong = [(cid, got, code) for cid, got, code in replayed if got != code]
    assert not wrong, f"{len(wrong)} of {len(replayed)} cases changed their code (id, now, recorded): {wrong[:10]}"
