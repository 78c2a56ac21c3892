"""The calibrator's decisions that need no GPU: the options record (attribute, then environment variable, then default), when a
capture graph is recorded, how modules are grouped under a cache budget and dealt over the group calls."""
import dataclasses

import pytest

from ptq4vit_amd.utils.capture_graph import graph_wanted
from ptq4vit_amd.utils.quant_calib import CalibOptions, HessianQuantCalibrator, calib_options, deal_over_calls, plan_groups

ENV = ("P4V_ARCH_GRAPHS", "P4V_CAPTURE_LANES", "P4V_SEARCH_STREAMS", "P4V_GROUPED", "P4V_GROUP_CALLS", "P4V_GROUP_GIB",
       "P4V_SHARD_CAPTURE", "P4V_CAPTURE_TRACE")

# (field, attribute or None, environment variable or None, [(attribute value, variable value, expected)]) -- the expectations are
# what the reads at the points of use gave before there was a record: `int(attr or env(.., "3"))`, `attr or int(env(.., "4"))`,
# `env(.., "1") != "0"` when the attribute is None, `attr or int(env(.., "0"))`, `"1"` / `"0"` force and anything else is auto
KNOBS = [
    ("use_graph", "use_graph", None, [(None, None, None), (True, None, True), (False, None, False)]),
    ("capture_lanes", "capture_lanes", "P4V_CAPTURE_LANES", [(None, None, 3), (None, "2", 2), (1, "2", 1), (0, "2", 2)]),
    ("search_streams", "search_streams", "P4V_SEARCH_STREAMS", [(None, None, 4), (None, "2", 2), (1, "2", 1), (0, "3", 3)]),
    ("search_grouped", "search_grouped", "P4V_GROUPED",
     [(None, None, True), (None, "0", False), (None, "1", True), (None, "no", True), (False, "1", False), (True, "0", True)]),
    ("group_calls", "group_calls", "P4V_GROUP_CALLS", [(None, None, 0), (None, "2", 2), (3, "2", 3), (0, "2", 2), (None, "-1", -1)]),
    ("shard_capture", "shard_capture", "P4V_SHARD_CAPTURE",
     [(None, None, None), (None, "1", True), (None, "0", False), (None, "auto", None), (None, "yes", None),
      (False, "1", False), (True, "0", True)]),
    ("arch_graphs", None, "P4V_ARCH_GRAPHS", [(None, None, True), (None, "0", False), (None, "1", True)]),
    ("group_gib", None, "P4V_GROUP_GIB", [(None, None, 150.0), (None, "2.5", 2.5)]),
    ("capture_trace", None, "P4V_CAPTURE_TRACE", [(None, None, False), (None, "1", True), (None, "0", False)]),
]


def _options(monkeypatch, env=None, **attrs):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    cal = HessianQuantCalibrator(None, {}, None)
    for k, v in attrs.items():
        setattr(cal, k, v)
    return calib_options(cal)


def test_every_field_of_the_options_record_is_in_the_table():
    assert [f.name for f in dataclasses.fields(CalibOptions)] == [k[0] for k in KNOBS]


@pytest.mark.parametrize("field,attr,var,cases", KNOBS, ids=[k[0] for k in KNOBS])
def test_options_attribute_beats_environment_beats_default(monkeypatch, field, attr, var, cases):
    for attr_value, var_value, want in cases:
        got = getattr(_options(monkeypatch, env={var: var_value} if var_value is not None else None,
                               **({attr: attr_value} if attr else {})), field)
        assert got == want and type(got) is type(want), (field, attr_value, var_value, got)


def test_options_are_frozen_and_the_attributes_start_as_none(monkeypatch):
    cal = HessianQuantCalibrator(None, {}, None)
    assert all(getattr(cal, k[1]) is None for k in KNOBS if k[1])
    with pytest.raises(dataclasses.FrozenInstanceError):
        _options(monkeypatch).capture_lanes = 1


def test_number_of_group_calls(monkeypatch):
    small, large, never = (lambda: (512 << 20) - 1), (lambda: 512 << 20), None     # `never`: must not be asked
    assert _options(monkeypatch).n_group_calls(small) == 1
    assert _options(monkeypatch).n_group_calls(large) == 3
    assert _options(monkeypatch, group_calls=2).n_group_calls(never) == 2
    assert _options(monkeypatch, group_calls=-1).n_group_calls(large) == 3
    assert _options(monkeypatch, search_streams=1, group_calls=3).n_group_calls(never) == 1
    assert _options(monkeypatch, env={"P4V_SEARCH_STREAMS": "1", "P4V_GROUP_CALLS": "3"}).n_group_calls(never) == 1


@pytest.mark.parametrize("use_graph,n_sub,calibrations,want", [
    (None, 2, 0, False), (None, 2, 1, True), (None, 23, 0, False), (None, 23, 1, True), (None, 24, 0, True), (None, 24, 1, True),
    (True, 2, 0, True), (True, 2, 1, True), (True, 23, 0, True), (True, 23, 1, True), (True, 24, 0, True), (True, 24, 1, True),
    (False, 2, 0, False), (False, 2, 1, False), (False, 23, 0, False), (False, 23, 1, False), (False, 24, 0, False), (False, 24, 1, False),
])
def test_graph_wanted(monkeypatch, use_graph, n_sub, calibrations, want):
    assert graph_wanted(_options(monkeypatch, use_graph=use_graph), n_sub, calibrations) is want


def test_plan_groups():
    todo = ["a", "b", "c", "d", "e"]
    sizes = {"a": 4, "b": 4, "c": 9, "d": 1, "e": 3}
    assert plan_groups(todo, None, 8, True, False) == [["a"], ["b"], ["c"], ["d"], ["e"]]          # sequential: singletons
    assert plan_groups(todo, None, 8, False, True) == [todo]                                       # sharded: one group
    assert plan_groups([], None, 8, False, True) == [[]]                                           # ... even of nothing
    assert plan_groups(todo, sizes, 8, False, False) == [["a", "b"], ["c"], ["d", "e"]]            # greedy; c > budget: alone
    assert plan_groups(todo, sizes, 100, False, False) == [todo]
    assert plan_groups(todo, {}, 0, False, False) == [todo]                                        # unknown sizes count as 0
    assert plan_groups([], sizes, 8, False, False) == []
    # the re-plan after an out-of-memory error in ["a", "b"] with "a" already calibrated: what is left, under half the budget
    assert plan_groups(["b", "c", "d", "e"], sizes, 4, False, False) == [["b"], ["c"], ["d", "e"]]


def test_modules_of_one_kind_are_dealt_round_robin_in_network_order():
    names = ["conv", "qkv0", "mm0", "fc0", "qkv1", "mm1", "fc1", "qkv2", "mm2", "fc2", "head"]
    kinds = {n: ("Linear", (8, 48)) if n[:3] == "qkv" else ("MatMul", (8, 16)) if n[:2] == "mm" else
             ("Linear", (8, 192)) if n[:2] == "fc" else ("Other", n) for n in names}
    # sorted by kind (as text), then by position: Linear/192: fc0 fc1 fc2; Linear/48: qkv0 qkv1 qkv2; MatMul: mm0 mm1 mm2; conv; head
    assert deal_over_calls(names, kinds, 1) == [["fc0", "fc1", "fc2", "qkv0", "qkv1", "qkv2", "mm0", "mm1", "mm2", "conv", "head"]]
    assert deal_over_calls(names, kinds, 3) == [["fc0", "qkv0", "mm0", "conv"], ["fc1", "qkv1", "mm1", "head"], ["fc2", "qkv2", "mm2"]]
    assert deal_over_calls(names, kinds, 2) == [["fc0", "fc2", "qkv1", "mm0", "mm2", "head"], ["fc1", "qkv0", "qkv2", "mm1", "conv"]]
