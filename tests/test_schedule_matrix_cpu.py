"""The schedule-switch table (helpers.SCHEDULE_ROWS) that tests/test_gpu_schedule_matrix.py runs against the fp64 oracle: a
pairwise cover of the two levels of every factor, complete over engine.Options (a switch added later without a level in the
table fails here), and every row a valid set of options.  No GPU needed."""
import itertools

import pytest

from gnnome_assembly_amd import engine
from helpers import SCHEDULE_CALLER, SCHEDULE_FACTORS, SCHEDULE_FORWARD, SCHEDULE_ROWS, schedule_switches

CAPS = ("TN_SIDE_CAP", "SRC_SIDE_CAP")         # exercised by test_side_stream_schedule_and_per_call_caps_change_nothing_but_rounding


def test_every_pair_of_levels_of_every_two_factors_appears_in_a_row():
    assert len(SCHEDULE_ROWS) == 8
    for row in SCHEDULE_ROWS.values():
        assert set(row) == set(SCHEDULE_FACTORS)
        assert all(row[f] in lv for f, lv in SCHEDULE_FACTORS.items())
    missing = [(a, la, b, lb) for a, b in itertools.combinations(SCHEDULE_FACTORS, 2)
               for la in SCHEDULE_FACTORS[a] for lb in SCHEDULE_FACTORS[b]
               if not any(r[a] == la and r[b] == lb for r in SCHEDULE_ROWS.values())]
    assert not missing, missing


def test_the_table_names_every_switch_but_the_caps():
    switches = set(SCHEDULE_FACTORS) - set(SCHEDULE_CALLER)
    assert switches == set(engine._OPTION_NAMES) - set(CAPS), sorted(switches ^ (set(engine._OPTION_NAMES) - set(CAPS)))
    assert set(SCHEDULE_FORWARD) <= switches
    assert len(SCHEDULE_FACTORS) == 13 and set(SCHEDULE_CALLER) == {"inputs", "flat"}
    assert SCHEDULE_ROWS["r0"] == {f: lv[0] for f, lv in SCHEDULE_FACTORS.items()}          # the defaults
    assert SCHEDULE_ROWS["r1"] == {f: lv[1] for f, lv in SCHEDULE_FACTORS.items()}          # everything changed


@pytest.mark.parametrize("row", sorted(SCHEDULE_ROWS))
def test_every_row_is_a_valid_set_of_options(row):
    sw = schedule_switches(SCHEDULE_ROWS[row])
    o = engine.current().replace(**sw)
    assert all(getattr(o, k) == v for k, v in sw.items())
    with engine.options(**sw) as o2:
        assert repr(o2) == repr(o)
