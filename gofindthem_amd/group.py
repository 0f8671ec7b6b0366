"""Python mirror of the reference's group finder (group/finder/finder.go) over libgft.so's gft_group_* C ABI
(SURVEY.md 8(f) row 2).  Same names and error behaviour; Go `error` values surface as GroupFinderError.

The object walk of group/finder/internal.go is the C++ side's job (csrc/group_host.cpp): every string leaf of every
document of a call goes through the finder as ONE batch on the GPU.  Python objects are handed over as JSON, which
is exactly the shape the walk understands (dict -> "key", list -> "index(i)", str -> a leaf); for plain objects only
attributes with an upper-case first letter are visible, like exported Go struct fields (internal.go:47-49).
"""
import ctypes as C
import json

import numpy as np

from . import _lib
from .engine import pack
from .finder import Finder


class GroupFinderError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def _jsonable(obj):
    """the part of a Python value the reference's reflect walk would see, as JSON-compatible data"""
    if isinstance(obj, str):
        return obj
    if isinstance(obj, dict):
        if any(not isinstance(k, str) for k in obj):
            return None                       # a Go map whose key type is not string is not walked (internal.go:62-64)
        return {k: _jsonable(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_jsonable(v) for v in obj]
    if isinstance(obj, (bool, int, float)) or obj is None:
        return None                           # not taggable; the value itself is irrelevant
    if hasattr(obj, "__dict__"):
        return {k: _jsonable(v) for k, v in vars(obj).items() if k[:1].isupper()}
    return None


def _json_call(fn, *args):
    """the out/cap/needed convention of the JSON-returning entry points"""
    need = C.c_uint64(0)
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        rc = fn(*args, C.cast(buf, C.c_void_p), cap, C.byref(need))
        if rc == _lib.GFT_E_INVALID and need.value > cap:
            cap = int(need.value)
            continue
        return rc, buf.value.decode("utf-8", "replace")


def dsl_parse(expr):
    """group/dsl Parser.Parse: {"tree":..,"tags":[..],"fields":[..]} or {"error": <reference text>} (host only)"""
    e = expr.encode("utf-8")
    rc, doc = _json_call(_lib.load().gft_group_dsl_parse, e, len(e))
    assert rc == 0
    return json.loads(doc)


def dsl_tokens(expr):
    e = expr.encode("utf-8")
    rc, doc = _json_call(_lib.load().gft_group_dsl_tokens, e, len(e))
    assert rc == 0
    return json.loads(doc)


class GroupFinder:
    """group/finder.GroupFinder.  NewFinder(findthem) / NewFinderWithRules(findthem, rulesByName)."""

    def __init__(self, findthem: Finder):
        self._L = _lib.load()
        self.findthem = findthem
        h = C.c_void_p()
        rc = self._L.gft_group_create(C.byref(h), findthem._h)
        if rc != 0:
            raise GroupFinderError(rc, "gft_group_create failed")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.gft_group_destroy(self._h)
            self._h = None

    __del__ = close

    def _err(self, rc):
        return GroupFinderError(rc, self._L.gft_group_last_error(self._h).decode("utf-8", "replace"))

    # -- rules (finder.go:45-85) -----------------------------------------------------------------------
    def AddRule(self, ruleName, expressions):
        n = ruleName.encode("utf-8")
        for raw in expressions:
            e = raw.encode("utf-8")
            rc = self._L.gft_group_add_rule(self._h, n, len(n), e, len(e))
            if rc != 0:
                raise self._err(rc)

    def AddRules(self, rulesByName):
        for k, v in rulesByName.items():
            self.AddRule(k, v)

    def state(self):
        """{"rules": {name: [{"ExpressionString", "Expression"}]}, "fields": [..], "tags": [..]}"""
        rc, doc = _json_call(self._L.gft_group_state, self._h)
        if rc != 0:
            raise self._err(rc)
        return json.loads(doc)

    def GetFieldNames(self):
        return self.state()["fields"]

    # -- tagging + rules over batches -------------------------------------------------------------------
    def _process(self, raws, includePaths, excludePaths, what):
        raws = [r.encode("utf-8") if isinstance(r, str) else bytes(r) for r in raws]
        blob, off = pack(raws)
        inc = json.dumps(list(includePaths)).encode() if includePaths else None
        exc = json.dumps(list(excludePaths)).encode() if excludePaths else None
        need = C.c_uint64(0)
        cap = max(1 << 16, 2 * int(blob.size))
        buf = C.create_string_buffer(cap)
        rc = self._L.gft_group_process_jsons(self._h, blob.ctypes.data, off.ctypes.data, len(raws), inc, len(inc) if inc else 0,
                                             exc, len(exc) if exc else 0, what, C.cast(buf, C.c_void_p), cap, C.byref(need))
        if rc == _lib.GFT_E_INVALID and need.value > cap:      # the library kept the document: fetch it, no second run
            cap = int(need.value)
            buf = C.create_string_buffer(cap)
            rc = self._L.gft_group_last_result(self._h, C.cast(buf, C.c_void_p), cap, C.byref(need))
        if rc != 0:
            raise self._err(rc)
        return json.loads(buf.value.decode("utf-8", "replace"))

    def ProcessJsons(self, rawJsons, includePaths=None, excludePaths=None):
        """batch extension of ProcessJson: one {"rules": {rule: [expressions]}} or {"error": ..} per document"""
        return self._process(rawJsons, includePaths, excludePaths, 0)

    def TagJsons(self, rawJsons, includePaths=None, excludePaths=None):
        return self._process(rawJsons, includePaths, excludePaths, 1)

    @staticmethod
    def _one(res, key):
        if "error" in res:
            raise GroupFinderError(_lib.GFT_E_ENGINE, res["error"])
        return res[key]

    def TagJson(self, data, includePaths=None, excludePaths=None):                 # finder.go:80-92
        return self._one(self.TagJsons([data], includePaths, excludePaths)[0], "tags")

    def TagObject(self, data, includePaths=None, excludePaths=None):               # finder.go:95-103
        return self.TagJson(json.dumps(_jsonable(data)), includePaths, excludePaths)

    def TagText(self, data):                                                       # finder.go:106-121
        return {tag: fields[""] for tag, fields in self.TagObject(data).items() if fields.get("")}

    def EvaluateRules(self, matchedExpByFieldByTag):                               # finder.go:118-137
        doc = json.dumps({t: ({f: sorted(v or ()) for f, v in fs.items()} if fs else None)
                          for t, fs in matchedExpByFieldByTag.items()}).encode()
        rc, out = _json_call(self._L.gft_group_evaluate, self._h, doc, len(doc))
        if rc != 0:
            raise self._err(rc)
        return json.loads(out)

    def ProcessJson(self, rawJson, includePaths=None, excludePaths=None):          # finder.go:160-172
        return self._one(self.ProcessJsons([rawJson], includePaths, excludePaths)[0], "rules")

    def ProcessObject(self, obj, includePaths=None, excludePaths=None):            # finder.go:180-190
        return self.ProcessJson(json.dumps(_jsonable(obj)), includePaths, excludePaths)

    def ProcessText(self, data):                                                   # finder.go:186-196
        return self.ProcessObject(data)

    # -- records: columns of strings instead of JSON documents, rules evaluated on the device -----------------
    def SetSchema(self, paths, includePaths=None, excludePaths=None):
        """the field paths of the record form ("Body", "Meta.Notes", "items.index(2)", "" for TagText), unique"""
        raws = [p.encode("utf-8") if isinstance(p, str) else bytes(p) for p in paths]
        blob, off = pack(raws)
        inc = json.dumps(list(includePaths)).encode() if includePaths else None
        exc = json.dumps(list(excludePaths)).encode() if excludePaths else None
        rc = self._L.gft_group_set_schema(self._h, blob.ctypes.data, off.ctypes.data, len(raws), inc, len(inc) if inc else 0,
                                          exc, len(exc) if exc else 0)
        if rc != 0:
            raise self._err(rc)
        self._schema = {p: i for i, p in enumerate(raws)}

    def rule_exprs(self):
        """[(rule name, expression string)] in the order of the rule bitmap's bits"""
        out = []
        name, expr, nl, el = C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint32()
        for i in range(self._L.gft_group_n_rule_exprs(self._h)):
            rc = self._L.gft_group_rule_expr(self._h, i, C.byref(name), C.byref(nl), C.byref(expr), C.byref(el))
            if rc != 0:
                raise self._err(rc)
            out.append((C.string_at(name.value, nl.value).decode("utf-8", "replace") if nl.value else "",
                        C.string_at(expr.value, el.value).decode("utf-8", "replace") if el.value else ""))
        return out

    def rule_words(self):
        return (self._L.gft_group_n_rule_exprs(self._h) + 31) // 32

    def pack_records(self, records):
        """[[(path or field index, str)]] -> (text_blob with slack, leaf_off, leaf_field, rec_off)"""
        schema = getattr(self, "_schema", None)
        if schema is None:
            raise GroupFinderError(_lib.GFT_E_INVALID, "no schema set (SetSchema)")
        texts, fields, rec_off = [], [], [0]
        for rec in records:
            for field, text in rec:
                if not isinstance(field, (int, np.integer)):
                    key = field.encode("utf-8") if isinstance(field, str) else bytes(field)
                    if key not in schema:
                        raise GroupFinderError(_lib.GFT_E_INVALID, "field path %r is not in the schema" % (field,))
                    field = schema[key]
                fields.append(int(field))
                texts.append(text.encode("utf-8") if isinstance(text, str) else bytes(text))
            rec_off.append(len(texts))
        blob, off = pack(texts)
        blob = np.concatenate([blob, np.zeros(64, dtype=np.uint8)])          # the readable slack every scan wants
        return blob, off, np.asarray(fields, dtype=np.uint32), np.asarray(rec_off, dtype=np.uint64)

    def ProcessRecordsBitmap(self, blob, leaf_off, leaf_field, rec_off):
        """host arrays of the record form -> the dense rule bitmap u32[n_records, ceil(R / 32)]"""
        n_records, n_leaves = len(rec_off) - 1, len(leaf_field)
        out = np.zeros((n_records, self.rule_words()), dtype=np.uint32)
        rc = self._L.gft_group_process_records(self._h, blob.ctypes.data, leaf_off.ctypes.data, leaf_field.ctypes.data, rec_off.ctypes.data,
                                               n_records, n_leaves, out.ctypes.data)
        if rc != 0:
            raise self._err(rc)
        return out

    def rules_from_bitmap(self, bitmap):
        """rows of the rule bitmap -> one expressionsByRule dict per record"""
        names = self.rule_exprs()
        res = []
        for row in np.asarray(bitmap):
            d = {}
            for w, word in enumerate(row):
                word = int(word)
                while word:
                    b = (word & -word).bit_length() - 1
                    word &= word - 1
                    name, expr = names[w * 32 + b]
                    d.setdefault(name, []).append(expr)
            res.append(d)
        return res

    def ProcessRecords(self, records):
        """records: a list of lists of (path or field index, str).  One expressionsByRule dict per record, what ProcessObject
        gives for an object with exactly those leaves."""
        return self.rules_from_bitmap(self.ProcessRecordsBitmap(*self.pack_records(records)))

    def ProcessRecordsDevice(self, text, leaf_off, leaf_field, rec_off):
        """torch device tensors (uint8 text with 64 bytes of slack, leaf_off / rec_off as 64-bit, leaf_field as 32-bit integers) ->
        the rule bitmap as a device tensor int32[n_records, ceil(R / 32)] (the bits of the u32 words)"""
        import torch
        n_records, n_leaves = int(rec_off.numel()) - 1, int(leaf_field.numel())
        for t, size in ((text, 1), (leaf_off, 8), (leaf_field, 4), (rec_off, 8)):
            if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
                raise GroupFinderError(_lib.GFT_E_INVALID, "ProcessRecordsDevice takes contiguous device tensors of 1, 8, 4 and 8 byte integers")
        out = torch.zeros((max(n_records, 0), self.rule_words()), dtype=torch.int32, device=text.device)
        torch.cuda.current_stream(text.device).synchronize()          # (the library runs on the engine's own stream)
        rc = self._L.gft_group_process_records_device(self._h, text.data_ptr(), leaf_off.data_ptr(), leaf_field.data_ptr(), rec_off.data_ptr(),
                                                      n_records, n_leaves, out.data_ptr())
        if rc != 0:
            raise self._err(rc)
        return out

    def debug_eval_rules_device(self, hit_bitmap, n_exprs, leaf_field, rec_off):
        """gft_debug_eval_rules_device: the two rule kernels over a caller-supplied leaf bitmap (torch device tensors, int32 rows,
        int32 fields, int64 offsets) -> the rule bitmap as a device tensor"""
        import torch
        n_records, n_leaves = int(rec_off.numel()) - 1, int(leaf_field.numel())
        out = torch.zeros((max(n_records, 0), self.rule_words()), dtype=torch.int32, device=rec_off.device)
        torch.cuda.current_stream(rec_off.device).synchronize()
        rc = self._L.gft_debug_eval_rules_device(self._h, hit_bitmap.data_ptr(), n_exprs, leaf_field.data_ptr(), rec_off.data_ptr(),
                                                 n_records, n_leaves, out.data_ptr())
        if rc != 0:
            raise self._err(rc)
        return out

    def debug_eval_rules(self, hit_bitmap, n_exprs, leaf_field, rec_off):
        """gft_debug_eval_rules: the compiled device words on the host over a caller-supplied leaf bitmap (no device)"""
        hit_bitmap = np.ascontiguousarray(hit_bitmap, dtype=np.uint32)
        leaf_field = np.ascontiguousarray(leaf_field, dtype=np.uint32)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        n_records, n_leaves = len(rec_off) - 1, len(leaf_field)
        out = np.zeros((n_records, self.rule_words()), dtype=np.uint32)
        rc = self._L.gft_debug_eval_rules(self._h, hit_bitmap.ctypes.data, n_exprs, leaf_field.ctypes.data, rec_off.ctypes.data,
                                          n_records, n_leaves, out.ctypes.data)
        if rc != 0:
            raise self._err(rc)
        return out

    # -- tag entries: TagObject's map of every record as sparse (field, expression) lists (csrc/gft_tags.hip) -------------------
    GUARD = 8                                                  # words behind a cap in which nothing may be stored

    def tags_from_entries(self, row_off, ent_field, ent_expr):
        """the three columns of a tag result -> one {tag: {field path: [expression strings, sorted]}} per record: what TagObject
        gives for an object with exactly the record's (path, string) leaves"""
        schema = getattr(self, "_schema", None)
        if schema is None:
            raise GroupFinderError(_lib.GFT_E_INVALID, "no schema set (SetSchema)")
        paths = [p.decode("utf-8", "surrogateescape") for p in sorted(schema, key=schema.get)]
        pairs = self.findthem._pairs()
        row_off = [int(x) for x in np.asarray(row_off).reshape(-1)]
        ent_field, ent_expr = np.asarray(ent_field).reshape(-1), np.asarray(ent_expr).reshape(-1)
        out = []
        for r in range(len(row_off) - 1):
            sets = {}
            for k in range(row_off[r], row_off[r + 1]):
                expr, tag = pairs[int(ent_expr[k])]
                sets.setdefault(tag, {}).setdefault(paths[int(ent_field[k])], set()).add(expr)
            out.append({t: {f: sorted(v) for f, v in fs.items()} for t, fs in sets.items()})
        return out

    def _entries_host(self, fn, head, n_records, cap, want_tag):
        """the row_off / ent_* / cap / total part of the host-pointer tag calls -> (row_off, ent_field, ent_expr, ent_tag, total);
        cap None: counted first, the arrays sized by the total; the arrays are GUARD words longer than cap, filled with 0xA5"""
        row_off, total = np.zeros(n_records + 1, dtype=np.uint64), C.c_uint64(0)
        if cap is None:
            rc = fn(self._h, *head, row_off.ctypes.data, None, None, None, 0, C.byref(total))
            if rc != 0:
                raise self._err(rc)
            cap = int(total.value)
        cols = [np.full(cap + self.GUARD, 0xA5A5A5A5, dtype=np.uint32) for _ in range(3)]
        rc = fn(self._h, *head, row_off.ctypes.data, cols[0].ctypes.data, cols[1].ctypes.data, cols[2].ctypes.data if want_tag else None, cap,
                C.byref(total))
        if rc != 0:
            raise self._err(rc)
        return row_off, cols[0], cols[1], cols[2] if want_tag else None, int(total.value)

    def _entries_device(self, fn, head, n_records, cap, want_tag, dev):
        """... and of the device-pointer calls: device tensors int64[n_records + 1], int32[cap + GUARD] (the guard words hold -1)"""
        import torch
        row_off = torch.zeros(n_records + 1, dtype=torch.int64, device=dev)
        total = C.c_uint64(0)
        torch.cuda.current_stream(dev).synchronize()          # (the library runs on the engine's own stream)
        if cap is None:
            rc = fn(self._h, *head, row_off.data_ptr(), None, None, None, 0, C.byref(total))
            if rc != 0:
                raise self._err(rc)
            cap = int(total.value)
        cols = [torch.full((cap + self.GUARD,), -1, dtype=torch.int32, device=dev) for _ in range(3)]
        torch.cuda.current_stream(dev).synchronize()
        rc = fn(self._h, *head, row_off.data_ptr(), cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr() if want_tag else None, cap,
                C.byref(total))
        if rc != 0:
            raise self._err(rc)
        return row_off, cols[0], cols[1], cols[2] if want_tag else None, int(total.value)

    def debug_tag_entries(self, hit_bitmap, n_exprs, leaf_field, rec_off, cap=None, want_tag=True):
        """gft_debug_tag_entries: the contract of the tag kernels in plain loops on the host over a caller-supplied leaf bitmap (no
        device) -> (row_off u64[n + 1], ent_field, ent_expr, ent_tag u32[cap + GUARD], total)"""
        hit_bitmap = np.ascontiguousarray(hit_bitmap, dtype=np.uint32)
        leaf_field = np.ascontiguousarray(leaf_field, dtype=np.uint32)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        n_records, n_leaves = len(rec_off) - 1, len(leaf_field)
        head = (hit_bitmap.ctypes.data, n_exprs, leaf_field.ctypes.data, rec_off.ctypes.data, n_records, n_leaves)
        return self._entries_host(self._L.gft_debug_tag_entries, head, max(n_records, 0), cap, want_tag)

    def debug_tag_entries_device(self, hit_bitmap, n_exprs, leaf_field, rec_off, cap=None, want_tag=True):
        """gft_debug_tag_entries_device: the three tag launches over a caller-supplied leaf bitmap (torch device tensors, int32 rows,
        int32 fields, int64 offsets) -> device tensors as _entries_device, and the total"""
        n_records, n_leaves = int(rec_off.numel()) - 1, int(leaf_field.numel())
        head = (hit_bitmap.data_ptr(), n_exprs, leaf_field.data_ptr(), rec_off.data_ptr(), n_records, n_leaves)
        return self._entries_device(self._L.gft_debug_tag_entries_device, head, max(n_records, 0), cap, want_tag, rec_off.device)

    def TagRecordsEntries(self, blob, leaf_off, leaf_field, rec_off, cap=None, want_tag=True):
        """host arrays of the record form -> (row_off, ent_field, ent_expr, ent_tag, total) as debug_tag_entries"""
        n_records, n_leaves = len(rec_off) - 1, len(leaf_field)
        head = (blob.ctypes.data, leaf_off.ctypes.data, leaf_field.ctypes.data, rec_off.ctypes.data, n_records, n_leaves)
        return self._entries_host(self._L.gft_group_tag_records, head, max(n_records, 0), cap, want_tag)

    def TagRecords(self, records):
        """records: a list of lists of (path or field index, str).  One {tag: {field: [expressions]}} per record, what TagObject
        gives for an object with exactly those leaves."""
        row_off, ent_field, ent_expr, _, total = self.TagRecordsEntries(*self.pack_records(records), want_tag=False)
        return self.tags_from_entries(row_off, ent_field[:total], ent_expr[:total])

    def TagRecordsDevice(self, text, leaf_off, leaf_field, rec_off, cap=None, want_tag=True):
        """torch device tensors as for ProcessRecordsDevice -> (row_off int64[n + 1], ent_field, ent_expr, ent_tag int32[cap + GUARD],
        total) on the device; without a cap the batch is counted first and the arrays are sized by the total"""
        n_records, n_leaves = int(rec_off.numel()) - 1, int(leaf_field.numel())
        for t, size in ((text, 1), (leaf_off, 8), (leaf_field, 4), (rec_off, 8)):
            if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
                raise GroupFinderError(_lib.GFT_E_INVALID, "TagRecordsDevice takes contiguous device tensors of 1, 8, 4 and 8 byte integers")
        head = (text.data_ptr(), leaf_off.data_ptr(), leaf_field.data_ptr(), rec_off.data_ptr(), n_records, n_leaves)
        return self._entries_device(self._L.gft_group_tag_records_device, head, max(n_records, 0), cap, want_tag, text.device)

    def TagJsonsDevice(self, blob, doc_off, cap=None, want_tag=True):
        """torch device tensors as for JsonLeavesDevice -> ((row_off, ent_field, ent_expr, ent_tag, total) as TagRecordsDevice, status
        uint8[n]); the row of a document whose status is not 0 is empty"""
        import torch
        n = int(doc_off.numel()) - 1
        for t, size in ((blob, 1), (doc_off, 8)):
            if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
                raise GroupFinderError(_lib.GFT_E_INVALID, "TagJsonsDevice takes contiguous device tensors of 1 and 8 byte integers")
        status = torch.zeros(max(n, 0), dtype=torch.uint8, device=blob.device)
        head = (blob.data_ptr(), doc_off.data_ptr(), n, status.data_ptr())
        return self._entries_device(self._L.gft_group_tag_jsons_device, head, max(n, 0), cap, want_tag, blob.device), status

    # -- the result document of rule rows as text (csrc/rules_json.cpp, csrc/gft_result.hip) --------------------------------------
    TEXT_GUARD = 32                                            # bytes behind a cap in which nothing may be stored (they hold 0xA5)

    def debug_rules_json(self, bitmap, hole_len=None, cap=None):
        """gft_debug_rules_json: the contract of the result kernels in plain loops on the host (no device, no schema) over rule rows
        u32[n_docs, ceil(R / 32)] -> (text uint8[cap + TEXT_GUARD], out_off u64[n_docs + 1], total); cap None: counted first"""
        bitmap = np.ascontiguousarray(bitmap, dtype=np.uint32)
        n = int(bitmap.shape[0])
        holes = None if hole_len is None else np.ascontiguousarray(hole_len, dtype=np.uint64)
        out_off, total = np.zeros(n + 1, dtype=np.uint64), C.c_uint64(0)
        head = (bitmap.ctypes.data, n, holes.ctypes.data if holes is not None else None)
        if cap is None:
            rc = self._L.gft_debug_rules_json(self._h, *head, None, 0, out_off.ctypes.data, C.byref(total))
            if rc != 0:
                raise self._err(rc)
            cap = int(total.value)
        text = np.full(cap + self.TEXT_GUARD, 0xA5, dtype=np.uint8)
        rc = self._L.gft_debug_rules_json(self._h, *head, text.ctypes.data, cap, out_off.ctypes.data, C.byref(total))
        if rc != 0:
            raise self._err(rc)
        return text, out_off, int(total.value)

    def RulesJsonDevice(self, rule_bitmap, hole_len=None, cap=None):
        """torch device tensors: rule rows int32[n_docs, ceil(R / 32)] as ProcessJsonsDevice / ProcessRecordsDevice give them, hole
        lengths int64[n_docs] or None -> (text uint8[cap + TEXT_GUARD] with 0xA5 behind the cap, out_off int64[n_docs + 1], total)
        on the device; without a cap the batch is counted first and the text is sized by the total"""
        import torch
        dev = rule_bitmap.device
        n = int(rule_bitmap.shape[0])
        for t, size in ((rule_bitmap, 4),) + (((hole_len, 8),) if hole_len is not None else ()):
            if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
                raise GroupFinderError(_lib.GFT_E_INVALID, "RulesJsonDevice takes contiguous device tensors of 4 and 8 byte integers")
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        total = C.c_uint64(0)
        head = (rule_bitmap.data_ptr(), n, hole_len.data_ptr() if hole_len is not None else None)
        torch.cuda.current_stream(dev).synchronize()           # (the library runs on the engine's own stream)
        if cap is None:
            rc = self._L.gft_group_rules_json_device(self._h, *head, None, 0, out_off.data_ptr(), C.byref(total))
            if rc != 0:
                raise self._err(rc)
            cap = int(total.value)
        text = torch.full((cap + self.TEXT_GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        rc = self._L.gft_group_rules_json_device(self._h, *head, text.data_ptr(), cap, out_off.data_ptr(), C.byref(total))
        if rc != 0:
            raise self._err(rc)
        return text, out_off, int(total.value)

    # -- the tag result document as text (csrc/tags_json.cpp, csrc/gft_tagdoc.hip) ------------------------------------------------
    def debug_tags_json(self, hit_bitmap, n_exprs, leaf_field, rec_off, hole_len=None, cap=None):
        """gft_debug_tags_json: the contract of the tag document kernels in plain loops on the host (no device) over a leaf bitmap
        u32[n_leaves, ceil(E / 32)] and the record arrays -> (text uint8[cap + TEXT_GUARD], out_off u64[n_records + 1], total);
        cap None: counted first"""
        hit_bitmap = np.ascontiguousarray(hit_bitmap, dtype=np.uint32)
        leaf_field = np.ascontiguousarray(leaf_field, dtype=np.uint32)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        n, n_leaves = len(rec_off) - 1, len(leaf_field)
        holes = None if hole_len is None else np.ascontiguousarray(hole_len, dtype=np.uint64)
        out_off, total = np.zeros(max(n, 0) + 1, dtype=np.uint64), C.c_uint64(0)
        head = (hit_bitmap.ctypes.data, n_exprs, leaf_field.ctypes.data, rec_off.ctypes.data, n, n_leaves,
                holes.ctypes.data if holes is not None else None)
        if cap is None:
            rc = self._L.gft_debug_tags_json(self._h, *head, None, 0, out_off.ctypes.data, C.byref(total))
            if rc != 0:
                raise self._err(rc)
            cap = int(total.value)
        text = np.full(cap + self.TEXT_GUARD, 0xA5, dtype=np.uint8)
        rc = self._L.gft_debug_tags_json(self._h, *head, text.ctypes.data, cap, out_off.ctypes.data, C.byref(total))
        if rc != 0:
            raise self._err(rc)
        return text, out_off, int(total.value)

    def TagsJsonDevice(self, hit_bitmap, leaf_field, rec_off, hole_len=None, cap=None):
        """torch device tensors: a leaf bitmap int32[n_leaves, ceil(E / 32)], leaf fields int32[n_leaves], record offsets
        int64[n_records + 1], hole lengths int64[n_records] or None -> (text uint8[cap + TEXT_GUARD] with 0xA5 behind the cap,
        out_off int64[n_records + 1], total) on the device; without a cap the batch is counted first"""
        import torch
        dev = rec_off.device
        n, n_leaves = int(rec_off.numel()) - 1, int(leaf_field.numel())
        for t, size in ((hit_bitmap, 4), (leaf_field, 4), (rec_off, 8)) + (((hole_len, 8),) if hole_len is not None else ()):
            if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
                raise GroupFinderError(_lib.GFT_E_INVALID, "TagsJsonDevice takes contiguous device tensors of 4, 4, 8 and 8 byte integers")
        out_off = torch.zeros(max(n, 0) + 1, dtype=torch.int64, device=dev)
        total = C.c_uint64(0)
        head = (hit_bitmap.data_ptr(), leaf_field.data_ptr(), rec_off.data_ptr(), n, n_leaves, hole_len.data_ptr() if hole_len is not None else None)
        torch.cuda.current_stream(dev).synchronize()           # (the library runs on the engine's own stream)
        if cap is None:
            rc = self._L.gft_group_tags_json_device(self._h, *head, None, 0, out_off.data_ptr(), C.byref(total))
            if rc != 0:
                raise self._err(rc)
            cap = int(total.value)
        text = torch.full((cap + self.TEXT_GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        rc = self._L.gft_group_tags_json_device(self._h, *head, text.data_ptr(), cap, out_off.data_ptr(), C.byref(total))
        if rc != 0:
            raise self._err(rc)
        return text, out_off, int(total.value)

    def _result_call(self, fn, rawJsons, *lists):
        """a JSON batch through an entry point that leaves a result document (fetched again, not run again, when it is larger than
        the buffer)"""
        raws = [r.encode("utf-8") if isinstance(r, str) else bytes(r) for r in rawJsons]
        blob, off = pack(raws)
        need = C.c_uint64(0)
        cap = max(1 << 16, 2 * int(blob.size))
        buf = C.create_string_buffer(cap)
        extra = []
        for lst in lists:
            j = json.dumps(list(lst)).encode() if lst else None
            extra += [j, len(j) if j else 0]
        rc = fn(self._h, blob.ctypes.data, off.ctypes.data, len(raws), *extra, C.cast(buf, C.c_void_p), cap, C.byref(need))
        if rc == _lib.GFT_E_INVALID and need.value > cap:
            cap = int(need.value)
            buf = C.create_string_buffer(cap)
            rc = self._L.gft_group_last_result(self._h, C.cast(buf, C.c_void_p), cap, C.byref(need))
        if rc != 0:
            raise self._err(rc)
        return json.loads(buf.value.decode("utf-8", "replace"))

    def TagJsonsSchema(self, rawJsons):
        """TagJsons(rawJsons, include, exclude of SetSchema) with the documents decoded and tagged on the device where it decides them"""
        return self._result_call(self._L.gft_group_tag_jsons_schema, rawJsons)

    def TagJsonsAuto(self, rawJsons, includePaths=None, excludePaths=None):
        """TagJsons(rawJsons, includePaths, excludePaths) with the schema discovered from the batch on the device"""
        return self._result_call(self._L.gft_group_tag_jsons_auto, rawJsons, includePaths, excludePaths)

    # -- JSON decoded on the device against the schema (csrc/gft_json.hip) -----------------------------------------------
    def _json_leaves_host(self, fn, docs, leaf_cap=None, text_cap=None):
        """gft_debug_json_leaves_ref / gft_debug_emulate_json_leaves over a list of byte strings -> (status, rec_off, leaf_field,
        leaf_off, text, (leaves, text bytes)); caps given: arrays of exactly that size behind which nothing may be stored"""
        docs = [d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in docs]
        blob, off = pack(docs)
        blob = np.concatenate([blob, np.zeros(64, dtype=np.uint8)])
        n = len(docs)
        status, rec_off, totals = np.zeros(n, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
        if leaf_cap is None:
            rc = fn(self._h, blob.ctypes.data, off.ctypes.data, n, status.ctypes.data, rec_off.ctypes.data, None, None, 0, None, 0, totals.ctypes.data)
            if rc != 0:
                raise self._err(rc)
            leaf_cap, text_cap = int(totals[0]), int(totals[1])
        guard = 8
        leaf_field = np.full(leaf_cap + guard, 0xA5A5A5A5, dtype=np.uint32)
        leaf_off = np.full(leaf_cap + 1 + guard, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        text = np.full(text_cap + guard, 0xA5, dtype=np.uint8)
        rc = fn(self._h, blob.ctypes.data, off.ctypes.data, n, status.ctypes.data, rec_off.ctypes.data, leaf_field.ctypes.data,
                leaf_off.ctypes.data, leaf_cap, text.ctypes.data, text_cap, totals.ctypes.data)
        if rc != 0:
            raise self._err(rc)
        return status, rec_off, leaf_field, leaf_off, text, (int(totals[0]), int(totals[1]))

    def debug_json_leaves_ref(self, docs, leaf_cap=None, text_cap=None):
        return self._json_leaves_host(self._L.gft_debug_json_leaves_ref, docs, leaf_cap, text_cap)

    def debug_emulate_json_leaves(self, docs, leaf_cap=None, text_cap=None):
        return self._json_leaves_host(self._L.gft_debug_emulate_json_leaves, docs, leaf_cap, text_cap)

    def debug_json_schema_find(self, parent, key):
        """(child node or -1, its field index or -1) of trie node `parent` under the component `key` (b"": the node itself)"""
        field = C.c_int64(-1)
        node = self._L.gft_debug_json_schema_find(self._h, parent, key, len(key), C.byref(field))
        return int(node), int(field.value)

    def JsonLeavesDevice(self, blob, doc_off, leaf_cap=None, text_cap=None):
        """torch device tensors (uint8 JSON text with 64 bytes of slack, doc_off as 64-bit integers) -> the record form as device
        tensors (status uint8[n], rec_off int64[n + 1], leaf_field int32[L], leaf_off int64[L + 1], text uint8[T + 64]) and
        (L, T).  Without caps the batch is counted first and the arrays are sized by the totals."""
        import torch
        n = int(doc_off.numel()) - 1
        for t, size in ((blob, 1), (doc_off, 8)):
            if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
                raise GroupFinderError(_lib.GFT_E_INVALID, "JsonLeavesDevice takes contiguous device tensors of 1 and 8 byte integers")
        dev = blob.device
        status = torch.zeros(max(n, 0), dtype=torch.uint8, device=dev)
        rec_off = torch.zeros(max(n, 0) + 1, dtype=torch.int64, device=dev)
        totals = np.zeros(2, dtype=np.uint64)
        torch.cuda.current_stream(dev).synchronize()
        if leaf_cap is None:
            rc = self._L.gft_group_json_leaves_device(self._h, blob.data_ptr(), doc_off.data_ptr(), n, status.data_ptr(), rec_off.data_ptr(),
                                                      None, None, 0, None, 0, totals.ctypes.data)
            if rc != 0:
                raise self._err(rc)
            leaf_cap, text_cap = int(totals[0]), int(totals[1])
        guard = 8                                              # (behind the caps: nothing may be stored there)
        leaf_field = torch.full((leaf_cap + guard,), -1, dtype=torch.int32, device=dev)
        leaf_off = torch.full((leaf_cap + 1 + guard,), -1, dtype=torch.int64, device=dev)
        text = torch.zeros(text_cap + 64, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        rc = self._L.gft_group_json_leaves_device(self._h, blob.data_ptr(), doc_off.data_ptr(), n, status.data_ptr(), rec_off.data_ptr(),
                                                  leaf_field.data_ptr(), leaf_off.data_ptr(), leaf_cap, text.data_ptr(), text_cap,
                                                  totals.ctypes.data)
        if rc != 0:
            raise self._err(rc)
        return status, rec_off, leaf_field, leaf_off, text, (int(totals[0]), int(totals[1]))

    def ProcessJsonsDevice(self, blob, doc_off):
        """torch device tensors as for JsonLeavesDevice -> (rule bitmap int32[n, ceil(R / 32)], status uint8[n]) on the device; the
        row of a document whose status is not 0 is that of an empty record"""
        import torch
        n = int(doc_off.numel()) - 1
        for t, size in ((blob, 1), (doc_off, 8)):
            if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
                raise GroupFinderError(_lib.GFT_E_INVALID, "ProcessJsonsDevice takes contiguous device tensors of 1 and 8 byte integers")
        out = torch.zeros((max(n, 0), self.rule_words()), dtype=torch.int32, device=blob.device)
        status = torch.zeros(max(n, 0), dtype=torch.uint8, device=blob.device)
        torch.cuda.current_stream(blob.device).synchronize()
        rc = self._L.gft_group_process_jsons_device(self._h, blob.data_ptr(), doc_off.data_ptr(), n, status.data_ptr(), out.data_ptr())
        if rc != 0:
            raise self._err(rc)
        return out, status

    def ProcessJsonLinesDevice(self, buf, length):
        """a resident blob of JSON Lines (a torch.uint8 device tensor of at least length + 64 bytes) -> (doc_off int64 [n + 1], rule
        bitmap int32 [n, ceil(R / 32)], status uint8 [n]) on the device: the blob is cut into a document per non-blank line on the
        device (SPLIT_JSON_LINES), then ProcessJsonsDevice runs over the result.  A schema must be set.  The tag side needs
        nothing of its own: TagJsonsDevice takes the offsets of split_lines_device as they are"""
        off = self.findthem.SplitLinesDevice(buf, length, 1)
        out, status = self.ProcessJsonsDevice(buf, off)
        return off, out, status

    # -- the documents whose rules fired (csrc/gft_select.hip) ----------------------------------------------------------------
    def rule_mask(self, rules=None):
        """the host mask of the select calls over rule rows: rule_words() uint32 words with the bits of rule_exprs() whose rule name
        is in `rules` -- ANY over them means "one of these rules fired".  None: every rule.  A name no rule has is a ValueError"""
        names = [r for r, _ in self.rule_exprs()]
        w = np.zeros((len(names) + 31) // 32, dtype=np.uint32)
        if rules is None:
            wanted = set(names)
        else:
            wanted = set([rules] if isinstance(rules, str) else rules)
            for r in wanted:
                if r not in names:
                    raise ValueError("rule_mask: no rule %r" % (r,))
        for i, r in enumerate(names):
            if r in wanted:
                w[i >> 5] |= np.uint32(1 << (i & 31))
        return w

    def SelectJsonLinesDevice(self, buf, length, rules=None, mode="any", keep_undecided=True):
        """a resident blob of JSON Lines -> the lines whose rules fired: ProcessJsonLinesDevice, then the select over the rule rows
        with rule_mask(rules).  keep_undecided: a document whose status is not 0 -- the device did not decide it, its row is that
        of an empty record -- is selected whatever its row says (its index in doc_idx tells which it was).  Returns (out uint8,
        out_off int64 [m + 1], doc_idx int64 [m], status uint8 [n]) on the device; a document carries its trailing whitespace and
        newline, so `out` is JSON Lines again.  A schema must be set"""
        from .engine import select_docs_tensor
        off, rows, status = self.ProcessJsonLinesDevice(buf, length)
        n_cols = int(self._L.gft_group_n_rule_exprs(self._h))
        eh = self.findthem.engine_handle()

        def call(*a):
            rc = self._L.gft_select_docs_device(eh, *a)
            if rc != 0:
                raise GroupFinderError(rc, self._L.gft_last_error(eh).decode("utf-8", "replace"))
        out, out_off, doc_idx = select_docs_tensor(call, buf, off, rows, n_cols, self.rule_mask(rules), mode, status if keep_undecided else None)
        return out, out_off, doc_idx, status

    def SelectJsonLines(self, data, rules=None, mode="any"):
        """the host-memory form: bytes -> (the selected lines as bytes, out_off uint64 [m + 1], doc_idx uint64 [m], undecided
        uint64 [u]).  One upload; the lines the device decided come back selected by their rows, the ones it did not decide (status
        not 0) come back too and `undecided` lists their input indices (a subset of doc_idx) -- the caller gives those to
        ProcessJsons.  The bytes are JSON Lines again.  A schema must be set"""
        import torch
        data = bytes(data)
        f = self.findthem
        dev = torch.device("cuda", f._device if f._device >= 0 else torch.cuda.current_device())
        buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
        if data:
            buf[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
        out, out_off, doc_idx, status = self.SelectJsonLinesDevice(buf, len(data), rules, mode, True)
        undecided = torch.nonzero(status, as_tuple=False).reshape(-1)
        return (out.cpu().numpy().tobytes(), out_off.cpu().numpy().astype(np.uint64), doc_idx.cpu().numpy().astype(np.uint64),
                undecided.cpu().numpy().astype(np.uint64))

    # -- the documents of every rule (csrc/gft_route.hip) -------------------------------------------------------------------
    def route_rule_names(self, rules=None):
        """the buckets of the route calls over rule rows: the rule names in byte order (None: every rule; a name no rule has is a
        ValueError -- rule_mask's)"""
        names = sorted(set(r for r, _ in self.rule_exprs()) if rules is None else set([rules] if isinstance(rules, str) else rules),
                       key=lambda r: r.encode("utf-8"))
        for r in names:
            self.rule_mask([r])
        return names

    def RouteJsonLinesDevice(self, buf, length, rules=None, mode="every"):
        """a resident blob of JSON Lines -> the lines of every rule: ProcessJsonLinesDevice, then the route over the rule rows with
        one bucket per rule name in byte order (route_rule_names(rules); rule_mask of each).  The rest bucket is always on and the
        status bytes go in as `also`: a document the device did not decide lands in the last bucket, with the decided ones no rule
        fired for.  Returns (out uint8, out_off int64 [m + 1], doc_idx int64 [m]) on the device, (bucket_doc, bucket_byte) uint64
        [len(names) + 2] on the host, status uint8 [n] on the device and the names.  A schema must be set"""
        from .engine import route_docs_tensor
        names = self.route_rule_names(rules)
        off, rows, status = self.ProcessJsonLinesDevice(buf, length)
        n_cols = int(self._L.gft_group_n_rule_exprs(self._h))
        eh = self.findthem.engine_handle()

        def call(*a):
            rc = self._L.gft_route_docs_device(eh, *a)
            if rc != 0:
                raise GroupFinderError(rc, self._L.gft_last_error(eh).decode("utf-8", "replace"))
        out, out_off, doc_idx, bucket_doc, bucket_byte = route_docs_tensor(call, buf, off, rows, n_cols, [self.rule_mask([r]) for r in names], mode,
                                                                           True, status)
        return out, out_off, doc_idx, bucket_doc, bucket_byte, status, names

    def RouteJsonLines(self, data, rules=None, mode="every"):
        """the host-memory form: bytes -> (parts, idx, undecided): parts a list of bytes, the lines of every rule in the order of
        route_rule_names(rules) and the rest last; idx a list of uint64 arrays, their input line numbers; undecided uint64 [u], the
        lines the device did not decide (status not 0) -- all of them in the last part; the caller gives those to ProcessJsons.
        Every part is JSON Lines again.  A schema must be set"""
        import torch
        data = bytes(data)
        f = self.findthem
        dev = torch.device("cuda", f._device if f._device >= 0 else torch.cuda.current_device())
        buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
        if data:
            buf[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
        out, _, doc_idx, bucket_doc, bucket_byte, status, _ = self.RouteJsonLinesDevice(buf, len(data), rules, mode)
        out, doc_idx = out.cpu().numpy().tobytes(), doc_idx.cpu().numpy().astype(np.uint64)
        undecided = torch.nonzero(status, as_tuple=False).reshape(-1).cpu().numpy().astype(np.uint64)
        B = len(bucket_doc) - 1
        return ([out[int(bucket_byte[b]):int(bucket_byte[b + 1])] for b in range(B)],
                [doc_idx[int(bucket_doc[b]):int(bucket_doc[b + 1])].copy() for b in range(B)], undecided)

    def ProcessJsonLines(self, data, includePaths=None, excludePaths=None):
        """JSON Lines from host memory (gft_group_process_json_lines): bytes, a document a line -> the result of
        ProcessJsonsSchema over the lines when a schema is set (the lists must then be None), of ProcessJsonsAuto(lines,
        includePaths, excludePaths) otherwise.  The blob goes up once and is cut on the device"""
        data = bytes(data)
        blob = np.frombuffer(data + b"\0" * 64, dtype=np.uint8)
        inc = json.dumps(list(includePaths)).encode() if includePaths else None
        exc = json.dumps(list(excludePaths)).encode() if excludePaths else None
        need = C.c_uint64(0)
        cap = max(1 << 16, 2 * len(data))
        buf = C.create_string_buffer(cap)
        rc = self._L.gft_group_process_json_lines(self._h, blob.ctypes.data, len(data), inc, len(inc) if inc else 0, exc, len(exc) if exc else 0,
                                                  C.cast(buf, C.c_void_p), cap, C.byref(need))
        if rc == _lib.GFT_E_INVALID and need.value > cap:      # the library kept the document: fetch it, no second run
            cap = int(need.value)
            buf = C.create_string_buffer(cap)
            rc = self._L.gft_group_last_result(self._h, C.cast(buf, C.c_void_p), cap, C.byref(need))
        if rc != 0:
            raise self._err(rc)
        return json.loads(buf.value.decode("utf-8", "replace"))

    def ProcessJsonsSchema(self, rawJsons):
        """ProcessJsons(rawJsons, include, exclude of SetSchema) with the documents decoded on the device where it decides them"""
        raws = [r.encode("utf-8") if isinstance(r, str) else bytes(r) for r in rawJsons]
        blob, off = pack(raws)
        need = C.c_uint64(0)
        cap = max(1 << 16, 2 * int(blob.size))
        buf = C.create_string_buffer(cap)
        rc = self._L.gft_group_process_jsons_schema(self._h, blob.ctypes.data, off.ctypes.data, len(raws), C.cast(buf, C.c_void_p), cap,
                                                    C.byref(need))
        if rc == _lib.GFT_E_INVALID and need.value > cap:      # the library kept the document: fetch it, no second run
            cap = int(need.value)
            buf = C.create_string_buffer(cap)
            rc = self._L.gft_group_last_result(self._h, C.cast(buf, C.c_void_p), cap, C.byref(need))
        if rc != 0:
            raise self._err(rc)
        return json.loads(buf.value.decode("utf-8", "replace"))

    # -- the schema discovered from the batch (csrc/gft_json.hip: k_json_paths) ----------------------------------------------
    PATH_CAP, PATH_POOL = 16384, 8 << 20                     # what the device keeps at most: the caps that always suffice

    def _paths_call(self, fn, *args):
        """the paths_blob / path_off / needed / n_paths part of the three path calls -> a sorted list of byte strings"""
        blob_cap, path_cap = self.PATH_POOL, self.PATH_CAP
        needed = np.zeros(2, dtype=np.uint64)
        n = C.c_uint64(0)
        head, tail = args
        while True:
            blob = np.zeros(blob_cap, dtype=np.uint8)
            off = np.zeros(path_cap + 1, dtype=np.uint64)
            rc = fn(self._h, *head, blob.ctypes.data, blob_cap, off.ctypes.data, path_cap, needed.ctypes.data, C.byref(n), *tail)
            if rc == _lib.GFT_E_INVALID and (needed[0] > blob_cap or needed[1] > path_cap):     # (the reference knows no cap)
                blob_cap, path_cap = max(blob_cap, int(needed[0])), max(path_cap, int(needed[1]))
                continue
            break
        if rc != 0:
            raise self._err(rc)
        raw = blob[:int(needed[0])].tobytes()
        return [raw[int(off[i]):int(off[i + 1])] for i in range(int(n.value))]

    def JsonPathsDevice(self, blob, doc_off):
        """torch device tensors as for JsonLeavesDevice -> (the distinct paths of the batch's string values as byte strings, sorted
        bytewise, each once; the number of paths found and not kept).  Needs no schema."""
        import torch
        n = int(doc_off.numel()) - 1
        for t, size in ((blob, 1), (doc_off, 8)):
            if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
                raise GroupFinderError(_lib.GFT_E_INVALID, "JsonPathsDevice takes contiguous device tensors of 1 and 8 byte integers")
        torch.cuda.current_stream(blob.device).synchronize()
        dropped = C.c_uint64(0)
        paths = self._paths_call(self._L.gft_group_json_paths_device, (blob.data_ptr(), doc_off.data_ptr(), n), (C.byref(dropped),))
        return paths, int(dropped.value)

    def _paths_host(self, docs):
        docs = [d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in docs]
        blob, off = pack(docs)
        blob = np.concatenate([blob, np.zeros(64, dtype=np.uint8)])
        return blob, off, len(docs)

    def debug_emulate_json_paths(self, docs):
        """gft_debug_emulate_json_paths over a list of byte strings -> (paths, dropped, the hashes in the set, ascending)"""
        blob, off, n = self._paths_host(docs)
        hashes = np.zeros(1 << 16, dtype=np.uint64)
        dropped, n_hashes = C.c_uint64(0), C.c_uint64(0)
        paths = self._paths_call(self._L.gft_debug_emulate_json_paths, (blob.ctypes.data, off.ctypes.data, n),
                                 (C.byref(dropped), hashes.ctypes.data, hashes.size, C.byref(n_hashes)))
        return paths, int(dropped.value), [int(h) for h in hashes[:int(n_hashes.value)]]

    def debug_json_paths_ref(self, docs):
        """gft_debug_json_paths_ref: the paths of the string values of the documents that the host route's reader accepts"""
        blob, off, n = self._paths_host(docs)
        return self._paths_call(self._L.gft_debug_json_paths_ref, (blob.ctypes.data, off.ctypes.data, n), ())

    def ProcessJsonsAuto(self, rawJsons, includePaths=None, excludePaths=None):
        """ProcessJsons(rawJsons, includePaths, excludePaths) with the schema discovered from the batch on the device and the
        documents decoded there where the device decides them"""
        raws = [r.encode("utf-8") if isinstance(r, str) else bytes(r) for r in rawJsons]
        blob, off = pack(raws)
        inc = json.dumps(list(includePaths)).encode() if includePaths else None
        exc = json.dumps(list(excludePaths)).encode() if excludePaths else None
        need = C.c_uint64(0)
        cap = max(1 << 16, 2 * int(blob.size))
        buf = C.create_string_buffer(cap)
        rc = self._L.gft_group_process_jsons_auto(self._h, blob.ctypes.data, off.ctypes.data, len(raws), inc, len(inc) if inc else 0,
                                                  exc, len(exc) if exc else 0, C.cast(buf, C.c_void_p), cap, C.byref(need))
        if rc == _lib.GFT_E_INVALID and need.value > cap:      # the library kept the document: fetch it, no second run
            cap = int(need.value)
            buf = C.create_string_buffer(cap)
            rc = self._L.gft_group_last_result(self._h, C.cast(buf, C.c_void_p), cap, C.byref(need))
        if rc != 0:
            raise self._err(rc)
        return json.loads(buf.value.decode("utf-8", "replace"))

    def json_auto_last(self):
        """(distinct paths, paths found and not kept, 1 if a schema was compiled) of the last ProcessJsonsAuto batch"""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._L.gft_group_json_auto_last(self._h, C.byref(a), C.byref(b), C.byref(c))
        return int(a.value), int(b.value), int(c.value)

    def json_last(self):
        """(documents decided on the device, documents handed to the host route) of the last ProcessJsonsSchema / ProcessJsonsAuto
        batch"""
        a, b = C.c_uint64(), C.c_uint64()
        self._L.gft_group_json_last(self._h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def last_batch(self):
        """(string leaves, text bytes) the last call sent through the finder"""
        a, b = C.c_uint64(), C.c_uint64()
        self._L.gft_group_last_batch(self._h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)


def NewFinder(findthem):
    return GroupFinder(findthem)


def NewFinderWithRules(findthem, rulesByName):
    g = GroupFinder(findthem)
    g.AddRules(rulesByName)
    return g


__all__ = ["GroupFinder", "GroupFinderError", "NewFinder", "NewFinderWithRules", "dsl_parse", "dsl_tokens"]
