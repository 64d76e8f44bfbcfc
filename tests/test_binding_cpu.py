"""CPU (-m "not gpu"): `_lib.SIGNATURES`, the Structure classes and the mirrored constants against include/vitseg.h.
The header is read with a small regex parser (below); only the last tests load the built library."""
import ctypes as C
import importlib
import os
import re

import pytest

from visiontransformer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# header scalar -> ctypes; a header type that is not here is reported by name, never skipped
SCALARS = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong,
           "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "int32_t": C.c_int32, "int64_t": C.c_int64}
STRUCTS = {"vitseg_config": _lib.CConfig, "vitseg_ce_options": _lib.CCEOptions, "vitseg_dice_options": _lib.CDiceOptions,
           "vitseg_augment_mask": _lib.CAugmentMask, "vitseg_tta_view": _lib.CTTAView}


# ---- the parser ----

def _ctype(spelling, array=False):
    """'const float*' -> ('float', 1): the base type without qualifiers and the pointer depth (an array declarator adds one)."""
    return " ".join(spelling.replace("const", " ").replace("*", " ").split()), spelling.count("*") + int(array)


def parse_header(text):
    """(declarations {name: (return type, [parameter types])}, structs {name: [(field, type)]},
    enums {name: [(member, value)]}, defines {name: int}); a type is `_ctype`'s pair."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)   # comments first: they hold parentheses and mentions of vitseg_x(...)
    text = re.sub(r"//[^\n]*", " ", text)
    defines = {k: int(v) for k, v in re.findall(r"^\s*#\s*define\s+(VITSEG_\w+)\s+(-?\d+)\s*$", text, flags=re.M)}
    text = " ".join(re.sub(r"^\s*#.*$", " ", text, flags=re.M).split())
    decls = {}
    # the look-behind leaves the previous declaration's `;` unconsumed: consecutive declarations share it
    for ret, name, args in re.findall(r"(?<=[;{}]) ?([A-Za-z_][\w ]*?[\w*]) ?\b(vitseg_\w+) ?\(([^()]*)\)(?= ?;)", text):
        params = []
        for p in ([] if args.strip() == "void" else args.split(",")):
            m = re.fullmatch(r"(.*?[\s*])(\w+)\s*((?:\[\w*\])?)", p.strip())
            assert m, f"{name}: cannot read the parameter {p!r}"
            params.append(_ctype(m.group(1), array=bool(m.group(3))))
        decls[name] = (_ctype(ret), params)
    structs = {}
    for name, body, alias in re.findall(r"typedef struct (\w+) ?\{([^{}]*)\} ?(\w+) ?;", text):
        assert name == alias, (name, alias)
        fields = []
        for f in filter(None, (f.strip() for f in body.split(";"))):
            m = re.fullmatch(r"(.*?[\s*])(\w+(?:\s*,\s*\w+)*)", f)   # `int32_t src_is_i64, out_is_i64`: several declarators
            assert m, f"struct {name}: cannot read the field {f!r}"
            fields += [(d.strip(), _ctype(m.group(1))) for d in m.group(2).split(",")]
        structs[name] = fields
    enums = {}
    for name, body in re.findall(r"\benum (\w+) ?\{([^{}]*)\}", text):
        members, value = [], -1
        for item in filter(None, (i.strip() for i in body.split(","))):
            member, _, explicit = (s.strip() for s in item.partition("="))
            value = int(explicit) if explicit else value + 1
            members.append((member, value))
        enums[name] = members
    return decls, structs, enums, defines


@pytest.fixture(scope="module")
def header():
    return parse_header(open(os.path.join(ROOT, "include", "vitseg.h")).read())


def table(signatures=None):
    """{name: (restype, argtypes)} of `_lib.SIGNATURES` (or a perturbed copy of it)."""
    return {name: (restype, list(argtypes)) for _, _, rows in (signatures or _lib.SIGNATURES).values()
            for name, restype, argtypes in rows}


# ---- the comparison ----

def _type_error(ctype, htype, structs=STRUCTS):
    """None when the ctypes type states the header type (base, pointer depth), else what is wrong."""
    base, depth = htype
    if depth == 0:
        if base not in SCALARS:
            return f"header type {base!r} is not in the test's map"
        return None if ctype is SCALARS[base] else f"{ctype.__name__} for {base}"
    if ctype is C.c_void_p or (ctype is C.c_char_p and base == "char" and depth == 1):
        return None
    if not (isinstance(ctype, type) and issubclass(ctype, C._Pointer)):
        return f"{getattr(ctype, '__name__', ctype)} for the pointer {base}{'*' * depth}"
    want = structs.get(base, SCALARS.get(base))
    if want is None:
        return f"POINTER for {base}{'*' * depth}: the header type is not in the test's map"
    return None if depth == 1 and ctype._type_ is want else f"POINTER({ctype._type_.__name__}) for {base}{'*' * depth}"


def signature_errors(decls, tab, structs=STRUCTS):
    """Every difference between the header's declarations and a {name: (restype, argtypes)} table, one line each."""
    errors = [f"{n}: declared in the header, no row in the table" for n in sorted(set(decls) - set(tab))]
    errors += [f"{n}: a row in the table, not declared in the header" for n in sorted(set(tab) - set(decls))]
    for name in sorted(set(decls) & set(tab)):
        (ret, params), (restype, argtypes) = decls[name], tab[name]
        want = C.c_char_p if ret == ("char", 1) else SCALARS.get(ret[0]) if ret[1] == 0 else None
        if want is None:
            errors.append(f"{name}: return type {ret} is not in the test's map")
        elif restype is not want:
            errors.append(f"{name}: restype {getattr(restype, '__name__', restype)}, the header returns {ret[0]}")
        if len(params) != len(argtypes):
            errors.append(f"{name}: {len(argtypes)} argtypes, the header has {len(params)} parameters")
            continue
        for i, (ctype, htype) in enumerate(zip(argtypes, params)):
            e = _type_error(ctype, htype, structs)
            if e:
                errors.append(f"{name}: argument {i}: {e}")
    return errors


def struct_errors(fields, cls):
    """Every difference between a header struct's [(field, type)] and a Structure class: names, order, types."""
    got = list(cls._fields_)
    if [f for f, _ in fields] != [f for f, _ in got]:
        return [f"{cls.__name__}: fields {[f for f, _ in got]}, the header has {[f for f, _ in fields]}"]
    return [f"{cls.__name__}.{f}: {e}" for (f, htype), (_, ctype) in zip(fields, got) for e in [_type_error(ctype, htype)] if e]


# ---- header against table: no library needed ----

def test_every_declaration_has_its_row_with_the_header_types(header):
    decls = header[0]
    assert len(decls) >= 130, len(decls)   # a parser that finds too little must not pass vacuously
    tab = table()
    assert len(tab) == sum(len(rows) for _, _, rows in _lib.SIGNATURES.values())   # no name twice
    assert set(decls) == set(tab), set(decls) ^ set(tab)
    errors = signature_errors(decls, tab)
    assert not errors, "\n".join(errors)
    returns = [decls[n][0] for n in decls]
    assert (returns.count(("int", 0)), returns.count(("size_t", 0)), returns.count(("char", 1))) == (len(decls) - 21, 20, 1)


def test_structure_classes_are_the_header_structs(header):
    structs = header[1]
    assert set(structs) == set(STRUCTS)
    errors = [e for name, cls in STRUCTS.items() for e in struct_errors(structs[name], cls)]
    assert not errors, "\n".join(errors)
    assert len(structs["vitseg_augment_mask"]) == 9   # the multi-declarator fields were all read


def test_constants_mirror_the_header(header):
    _, _, enums, defines = header
    assert len(enums) == 9
    checked = 0
    for name, members in enums.items():
        if name == "vitseg_kernel_kind":
            continue
        for member, value in members:
            assert member.startswith("VITSEG_"), member
            if member == "VITSEG_BUF_COUNT":   # the one member of these families `_lib` does not mirror
                continue
            assert getattr(_lib, member[len("VITSEG_"):]) == value, member
            checked += 1
    assert checked == 5 + 23 + 4 + 2 + 7 + 2 + 2 + 2   # status, T_*, precisions, BUF_*, SLICES_*, CONF_*, AUGMENT_* (two enums)
    kinds = enums["vitseg_kernel_kind"]
    assert kinds[-1][0] == "VITSEG_K_COUNT" and [v for _, v in kinds] == list(range(len(kinds)))
    assert _lib.KERNEL_KINDS == [m[len("VITSEG_K_"):].lower() for m, _ in kinds[:-1]]
    assert _lib.VERSION == defines["VITSEG_VERSION"]
    assert _lib.PROPS_FIELDS == defines["VITSEG_PROPS_FIELDS"]


def test_the_comparison_can_fail(header):
    """Each kind of mistake the tests above exist for, made on a copy, is reported."""
    decls, structs = header[0], header[1]

    def errors_after(change):
        tab = table()
        change(tab)
        return signature_errors(decls, tab)

    def edit(name, restype=None, args=None):
        def change(tab):
            r, a = tab[name]
            tab[name] = (restype or r, args(a) if args else a)
        return change
    assert signature_errors(decls, table()) == []
    e = errors_after(edit("vitseg_forward", args=lambda a: a[:-1]))   # a dropped argument
    assert e == ["vitseg_forward: 10 argtypes, the header has 11 parameters"]
    e = errors_after(edit("vitseg_forward", args=lambda a: a[:9] + [C.c_int] + a[10:]))   # c_int for a size_t
    assert e == ["vitseg_forward: argument 9: c_int for size_t"]
    e = errors_after(edit("vitseg_adam_step", args=lambda a: a[:9] + [C.c_uint32] + a[10:]))   # signedness
    assert e == ["vitseg_adam_step: argument 9: c_uint for int"]
    e = errors_after(edit("vitseg_forward", args=lambda a: a[:4] + [C.c_void_p] + a[5:]))   # a pointer for a scalar
    assert e == ["vitseg_forward: argument 4: c_void_p for int"]
    e = errors_after(edit("vitseg_forward", args=lambda a: [C.c_int] + a[1:]))   # a scalar for a pointer
    assert e == ["vitseg_forward: argument 0: c_int for the pointer vitseg_config*"]
    e = errors_after(edit("vitseg_forward", args=lambda a: [C.POINTER(_lib.CTTAView)] + a[1:]))   # another struct
    assert e == ["vitseg_forward: argument 0: POINTER(CTTAView) for vitseg_config*"]
    e = errors_after(edit("vitseg_get_option", args=lambda a: [a[0], C.POINTER(C.c_int)]))   # another pointee
    assert e == ["vitseg_get_option: argument 1: POINTER(c_int) for long long*"]
    e = errors_after(edit("vitseg_ce_scratch_bytes", restype=C.c_int))   # the default restype left on a size_t function
    assert e == ["vitseg_ce_scratch_bytes: restype c_int, the header returns size_t"]
    e = errors_after(lambda tab: tab.pop("vitseg_confidence"))
    assert e == ["vitseg_confidence: declared in the header, no row in the table"]
    e = errors_after(lambda tab: tab.update(vitseg_nothing=(C.c_int, [])))
    assert e == ["vitseg_nothing: a row in the table, not declared in the header"]
    e = signature_errors({**decls, "vitseg_version": (("short", 0), [("__int128", 0)])}, {**table(), "vitseg_version": (C.c_int, [C.c_int])})
    assert e == ["vitseg_version: return type ('short', 0) is not in the test's map",
                 "vitseg_version: argument 0: header type '__int128' is not in the test's map"]

    class Swapped(C.Structure):
        _fields_ = [_lib.CTTAView._fields_[i] for i in (0, 2, 1, 3)]

    class Narrow(C.Structure):
        _fields_ = [(f, C.c_int32 if f == "scratch_bytes" else t) for f, t in _lib.CDiceOptions._fields_]
    assert struct_errors(structs["vitseg_tta_view"], _lib.CTTAView) == []
    assert len(struct_errors(structs["vitseg_tta_view"], Swapped)) == 1
    assert struct_errors(structs["vitseg_dice_options"], Narrow) == ["Narrow.scratch_bytes: c_int for size_t"]


def test_the_parser_reads_what_the_header_is_written_in():
    decls, structs, enums, defines = parse_header("""
        #define VITSEG_VERSION 7 /* a comment with vitseg_old(int) in it,
                                    on two lines */
        enum vitseg_e { VITSEG_A = -2, VITSEG_B, VITSEG_C = 5 };   // vitseg_gone(void);
        typedef struct vitseg_s { const float* p; int32_t a, b; } vitseg_s;
        int vitseg_one(void);
        size_t vitseg_two(const vitseg_s* s,
                          const int R[4], long long v);
        const char* vitseg_three(uint8_t* out /* [n] or NULL */);""")
    assert decls == {"vitseg_one": (("int", 0), []),
                     "vitseg_two": (("size_t", 0), [("vitseg_s", 1), ("int", 1), ("long long", 0)]),
                     "vitseg_three": (("char", 1), [("uint8_t", 1)])}
    assert structs == {"vitseg_s": [("p", ("float", 1)), ("a", ("int32_t", 0)), ("b", ("int32_t", 0))]}
    assert enums == {"vitseg_e": [("VITSEG_A", -2), ("VITSEG_B", -1), ("VITSEG_C", 5)]}
    assert defines == {"VITSEG_VERSION": 7}


# ---- the public names read off the table ----

WORDS = {"at": "interpolated position embeddings", "region": "connected regions", "sdf": "distance transforms",
         "splitk": "the split-K entry points", "ce_opts": "the cross-entropy options", "helper": "the helper-kernel entry points",
         "window": "sliding-window inference", "dice": "the CE + Dice loss", "distance": "the boundary-distance metrics",
         "skeleton": "the skeletons", "augment": "the training augmentation", "tta": "test-time augmentation",
         "clean": "the mask clean-up", "match": "the region matching", "props": "the per-region measurements",
         "confidence": "the confidence scores"}


def test_name_lists_are_read_off_the_table():
    assert [k for k, (required, _, _) in _lib.SIGNATURES.items() if required] == ["core"]
    assert {k: what for k, (required, what, _) in _lib.SIGNATURES.items() if not required} == WORDS
    late = []
    for key in WORDS:
        names = getattr(_lib, f"{key.upper()}_EXPORTS")
        assert type(names) is list and names == [name for name, _, _ in _lib.SIGNATURES[key][2]]
        late += names
    assert type(_lib._LATE_EXPORTS) is list and _lib._LATE_EXPORTS == late
    assert type(_lib.EXPORTS) is list and _lib.EXPORTS == [name for name, _, _ in _lib.SIGNATURES["core"][2]] + late
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS)) == 131 and _lib.VERSION == 110


# ---- after lib(): these need the built library, as the other CPU tests do ----

def test_lib_binds_every_row():
    l = _lib.lib()
    for name, (restype, argtypes) in table().items():
        fn = getattr(l, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
        assert _lib.symbol(name) is fn


@pytest.mark.parametrize("key", list(WORDS))
def test_each_alias_names_its_feature_for_a_missing_symbol(key):
    msg = rf"has no vitseg_not_there \(built before {re.escape(WORDS[key])}\): rebuild it \(python -m visiontransformer_amd\.build\)"
    with pytest.raises(RuntimeError, match=msg):
        getattr(_lib, f"{key}_symbol")("vitseg_not_there")
    assert getattr(_lib, f"{key}_symbol")(_lib.SIGNATURES[key][2][0][0]) is not None


def test_symbol_names_the_feature_of_a_row_the_library_lacks(monkeypatch):
    class Old:   # a library built before the confidence scores
        def __getattr__(self, name):
            if name == "vitseg_confidence":
                raise AttributeError(name)
            return getattr(_lib._lib, name)
    _lib.lib()
    monkeypatch.setattr(_lib, "lib", Old)
    with pytest.raises(RuntimeError, match=r"has no vitseg_confidence \(built before the confidence scores\): rebuild it"):
        _lib.symbol("vitseg_confidence")
    with pytest.raises(RuntimeError, match=r"has no vitseg_nothing \(built before this entry point\): rebuild it"):
        _lib.symbol("vitseg_nothing")
    assert _lib.symbol("vitseg_regions") is _lib._lib.vitseg_regions


@pytest.mark.parametrize("module, test", [
    ("test_clean_cpu", "test_clean_mask_rejects_bad_arguments_before_the_library"),
    ("test_clean_cpu", "test_clean_mask_with_both_steps_off_returns_its_argument"),
    ("test_sdf_cpu", "test_compute_sdf_rejects_bad_arguments_before_the_library"),
    ("test_regions_cpu", "test_region_boxes_rejects_bad_arguments_before_the_library"),
    ("test_ce_options_cpu", "test_defaults_take_the_existing_symbols"),
    ("test_ce_dice_cpu", "test_lightning_without_dice_asks_for_no_new_symbol"),
])
def test_paths_that_must_not_reach_the_library_do_not_ask_symbol_either(monkeypatch, module, test):
    """These tests prove that a path asks the library for nothing by patching one group's alias.  The package asks
    `_lib.symbol` itself, so their bodies run once more with that patched as well."""
    def no_call(name, what=None):
        raise AssertionError(f"{name} requested")
    monkeypatch.setattr(_lib, "symbol", no_call)
    getattr(importlib.import_module(module), test)(monkeypatch)
