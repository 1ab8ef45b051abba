"""The three lazy dicts of the object surface (``chimeric_alignments``, ``large_indel_alignments``, ``read_length``) against
plain dicts: every ``dict`` operation on a fresh, unloaded container gives what it gives on a plain ``dict`` holding the
same entries, and leaves the same entries in the same order behind."""
import collections.abc as abc
import copy
import operator
import pickle
import types

import numpy as np
import pytest

from coral_amd import infer_breakpoint_graph as ibg

_OWNERS = []                  # the containers hold their owner through a weakref proxy: keep every owner alive


class _Names:
    def __init__(self, names):
        self.names = names

    def take(self, ids):
        return [self.names[i] for i in np.asarray(ids).tolist()]


class _Owner:
    """What the containers read on bam_to_breakpoint_nanopore."""

    def __init__(self):
        self.rec = types.SimpleNamespace(header_chroms=["chr1", "chr2"], names=_Names(["a", "b", "c", "d"]))
        self._names_of = self.rec.names.take
        self._hashed = False
        # three reads (rows of name_ids below), the second failed; SA segments 0-1 belong to the first, 2 to the third
        self._chim = types.SimpleNamespace(
            failed=np.array([False, True, False]), off=np.array([0, 2, 2, 3]),
            qs=np.array([0, 50, 10]), qe=np.array([40, 90, 60]), tid=np.array([0, 1, 0]), ra=np.array([100, 900, 300]),
            rb=np.array([140, 860, 350]), strand=np.array([0, 1, 0]), mapq=np.array([60, 20, 60]), nm=np.array([1.0, 2.5, 0.0]))
        _OWNERS.append(self)

    def _cniset(self, row):
        return {row, -1}


def chimeric():
    return ibg._ChimericAlignments(_Owner(), np.array([2, 0, 1]))            # keys c, a, b


def indel():
    return ibg._LazyIndelAlignments(_Owner(), np.array([0, 3]), np.array([0, 2, 3]), np.array([0, 0, 1]), np.array([10, 20, 30]),
                                    np.array([5, 15, 25]), np.array([1, 1, 2]), np.array([40, 40, 50]), np.array([60, 60, 20]))


def read_length():
    o = _Owner()
    return ibg._LazyReadLength(o.rec.names, types.SimpleNamespace(read_length=np.array([5, -1, 7, 9])))


MAKERS = [chimeric, indel, read_length]


def _first(r):
    return next(iter(r))


def _updated(d, x):
    d.update(x)
    return d


OPS = {
    "len": lambda x, r: len(x),
    "bool": lambda x, r: bool(x),
    "list": lambda x, r: list(x),
    "reversed": lambda x, r: list(reversed(x)),
    "contains": lambda x, r: [k in x for k in [*r, "zz"]],
    "keys": lambda x, r: x.keys(),
    "values": lambda x, r: x.values(),
    "items": lambda x, r: x.items(),
    "getitem": lambda x, r: [x[k] for k in r],
    "getitem missing": lambda x, r: x["zz"],
    "get": lambda x, r: [x.get(k) for k in r] + [x.get("zz"), x.get("zz", 0)],
    "setdefault existing": lambda x, r: x.setdefault(_first(r), 0),
    "setdefault new": lambda x, r: x.setdefault("zz", 0),
    "pop": lambda x, r: x.pop(_first(r)),
    "pop missing with default": lambda x, r: x.pop("zz", 0),
    "pop missing": lambda x, r: x.pop("zz"),
    "popitem": lambda x, r: x.popitem(),
    "popitem empty": lambda x, r: (x.clear(), x.popitem()),
    "setitem new": lambda x, r: x.__setitem__("zz", 1),
    "setitem then read": lambda x, r: (x.__setitem__(_first(r), 99), x[_first(r)]),
    "setitem None then read": lambda x, r: (x.__setitem__(_first(r), None), x[_first(r)], x.get(_first(r), 0)),
    "delitem": lambda x, r: x.__delitem__(_first(r)),
    "delitem missing": lambda x, r: x.__delitem__("zz"),
    "update kwargs": lambda x, r: x.update(zz=1),
    "update dict": lambda x, r: x.update({_first(r): 1, "zz": 2}),
    "update pairs": lambda x, r: x.update([("zz", 1)]),
    "ior": lambda x, r: operator.ior(x, {"zz": 1}) is x,
    "clear": lambda x, r: (x.clear(), len(x), list(x)),
    "copy": lambda x, r: x.copy(),
    "or empty": lambda x, r: x | {},
    "or": lambda x, r: x | {"zz": 1, _first(r): 2},
    "ror": lambda x, r: {"zz": 1, _first(r): 2} | x,
    "or not a dict": lambda x, r: x | 5,
    "fromkeys": lambda x, r: type(x).fromkeys("ab", 0),
    "eq": lambda x, r: x == r,
    "eq reflected": lambda x, r: r == x,
    "ne": lambda x, r: x != r,
    "ne reflected": lambda x, r: r != x,
    "eq empty": lambda x, r: (x == {}, {} == x, x != {}),
    "eq not a dict": lambda x, r: (x.__eq__(5), x.__ne__(5), x == 5),
    "repr": lambda x, r: repr(x),
    "str": lambda x, r: str(x),
    "hash": lambda x, r: hash(x),
    "pickle": lambda x, r: pickle.loads(pickle.dumps(x)),
    "copy.copy": lambda x, r: copy.copy(x),
    "copy.deepcopy": lambda x, r: copy.deepcopy(x),
    "splat": lambda x, r: {**x},
    "dict()": lambda x, r: dict(x),
    "plain update": lambda x, r: _updated({"zz": 1}, x),
    # keys loaded first, values not yet built
    "keys then items": lambda x, r: (list(x), list(x.items())),
    "keys then or": lambda x, r: (list(x), x | {}),
    "keys then popitem": lambda x, r: (list(x), x.popitem()),
    "keys then copy": lambda x, r: (list(x), x.copy()),
    "keys then eq": lambda x, r: (list(x), x == r, r == x),
    "keys then repr": lambda x, r: (list(x), repr(x)),
    "keys then pickle": lambda x, r: (list(x), pickle.loads(pickle.dumps(x))),
}


def _norm(v):
    if isinstance(v, (abc.KeysView, abc.ValuesView, abc.ItemsView, abc.Iterator)):
        return list(v)
    if type(v) is dict:
        return list(v.items())          # order included
    if isinstance(v, tuple):
        return tuple(_norm(e) for e in v)
    return v


def _outcome(op, x, ref):
    try:
        v = op(x, ref)
    except Exception as e:          # the same exception type as a plain dict raises (messages name the class)
        return "raises", type(e), e.args if isinstance(e, KeyError) else None
    return type(v), _norm(v)


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("make", MAKERS)
def test_behaves_like_a_plain_dict(make, op):
    x, plain = make(), dict(make().items())
    assert _outcome(OPS[op], x, dict(make().items())) == _outcome(OPS[op], plain, dict(make().items()))
    assert list(x.items()) == list(plain.items())


@pytest.mark.parametrize("make", MAKERS)
def test_two_lazy_dicts(make):
    plain = dict(make().items())
    assert make() == make() and not make() != make()
    assert list((make() | make()).items()) == list((plain | plain).items())
    x = make()
    x |= make()
    assert list(x.items()) == list(plain.items())


@pytest.mark.parametrize("make", MAKERS)
def test_len_and_bool_do_not_load(make):
    x = make()
    assert len(x) == len(dict(make().items())) and bool(x)
    assert not x._loaded


def test_chimeric_values_are_built_one_at_a_time():
    x = chimeric()
    assert x["a"] == ([], [], [])                                           # the failed read
    assert dict.__getitem__(x, "c") is x._PENDING
    assert x["c"] == ([[0, 40], [50, 90]], [["chr1", 100, 140, "+"], ["chr2", 900, 860, "-"]], [60, 20], [1.0, 2.5])


def test_invalidate_rebuilds_the_values_made_so_far():
    x = chimeric()
    x["c"]
    x["b"] = "mine"
    x["b"]
    x._owner._hashed = True
    x.invalidate()
    assert [seg[4] for seg in dict.__getitem__(x, "c")[1]] == [{0, -1}, {1, -1}]     # rebuilt with the CN-segment sets
    assert dict.__getitem__(x, "b") == "mine"                                          # a value written since is kept
    assert x["a"] == ([], [], [])


# names dict supplies that are not methods a container could leave to the empty table: the type machinery, and the order
# comparisons (dict's return NotImplemented, so ``<`` raises TypeError either way)
MACHINERY = {"__class__", "__new__", "__init__", "__init_subclass__", "__subclasshook__", "__class_getitem__", "__getattribute__",
             "__setattr__", "__delattr__", "__dir__", "__format__", "__sizeof__", "__reduce_ex__", "__doc__", "__str__",
             "__lt__", "__le__", "__gt__", "__ge__"}


def test_lazydict_overrides_every_dict_method():
    from coral_amd.lazysets import LazyDict
    assert [n for n in dir(dict) if n not in MACHINERY and n not in vars(LazyDict)] == []


def test_containers_only_load():
    from coral_amd.lazysets import LazyDict
    for cls in (ibg._ChimericAlignments, ibg._LazyIndelAlignments, ibg._LazyReadLength):
        assert issubclass(cls, LazyDict)
        assert sorted(set(vars(cls)) & set(dir(dict)) - {"__init__", "__doc__"}) == [], cls.__name__


def test_build_leaves_them_unloaded(golden_dir, tmp_path, monkeypatch):
    """Nothing in the graph build reads these containers: their Python objects are made only for a consumer after it."""
    from coral_amd import synth
    from coral_amd.lazysets import LazyDict
    from coral_amd.records import DeviceRecords
    from tests.product_check import install_cpu_kernel_fakes, load_case
    install_cpu_kernel_fakes(monkeypatch)
    gold, cfg, rec = load_case(golden_dir, "tiny")
    cn, seeds = str(tmp_path / "cn.bed"), str(tmp_path / "seeds.bed")
    synth.write_cn_bed(cfg, cn)
    synth.write_seed_bed(cfg, seeds)
    b = ibg.build_graph_from_records(DeviceRecords(rec, "cpu"), seeds, cn, None, min_bp_support=gold["min_bp_support"])
    want = {"read_length": gold["A3"]["n_read_length"], "chimeric_alignments": len(gold["A3"]["chimeric_alignments"]["__dict__"]),
            "large_indel_alignments": len(gold["A6"]["large_indel_alignments"]["__dict__"])}
    for name, n in want.items():
        x = getattr(b, name)
        assert isinstance(x, LazyDict) and not x._loaded, name
        assert len(x) == n and not x._loaded, name
