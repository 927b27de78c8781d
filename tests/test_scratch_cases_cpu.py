"""tests/scratch_cases.py kept complete without a GPU: every engine entry of include/vd_amd.h is a row or an exemption, every device
pointer of struct vd_engine is scratch or state and vd_scratch_fill fills exactly the scratch, and the rows served again from the
step's option matrix cover its axes.  Each cover is shown to fail on a list with one name removed."""
import collections

import scratch_cases as sk
import step_matrix_cases as sm


def _read(path):
    with open(path) as f:
        return f.read()


def _without(d, key):
    return collections.OrderedDict((k, v) for k, v in d.items() if k != key)


def test_every_engine_entry_of_the_header_is_a_row_or_an_exemption():
    launch, other = sk.header_entries(_read(sk.HEADER))
    assert len(launch) >= 43 and len(other) >= 60 and "vd_p_sample" in launch and "vd_set_schedule" in other and "vd_scratch_fill" in other
    assert "vd_op_cfg_combine" not in launch + other                             # no engine: not this table's
    assert sk.entry_cover(launch, other, sk.ENTRIES, sk.EXEMPT) == []
    assert list(sk.ENTRIES) == [n for n in sk.ENTRIES if n in launch]            # a row is an entry that takes a stream
    for name, why in sk.EXEMPT.items():
        assert len(why.split()) >= 3, (name, "an exemption has a reason in words")
    # the mistakes the cover is there for
    assert sk.entry_cover(launch, other, _without(sk.ENTRIES, "vd_eps_vjp"), sk.EXEMPT) == ["vd_eps_vjp: launches work (vd_engine*, a stream) and is no row of ENTRIES"]
    assert sk.entry_cover(launch, other, sk.ENTRIES, _without(sk.EXEMPT, "vd_set_freeu")) == ["vd_set_freeu: in neither list"]
    both = collections.OrderedDict(sk.EXEMPT, vd_q_sample="also exempt, by mistake")
    assert sk.entry_cover(launch, other, sk.ENTRIES, both) == ["vd_q_sample: in ENTRIES and in EXEMPT"]
    new = "int vd_new_sampler(vd_engine* e, int B, float* out, void* stream);\nint vd_set_new(vd_engine* e, int on);\n"
    l2, o2 = sk.header_entries(_read(sk.HEADER) + new)
    assert sk.entry_cover(l2, o2, sk.ENTRIES, sk.EXEMPT) == ["vd_new_sampler: launches work (vd_engine*, a stream) and is no row of ENTRIES", "vd_set_new: in neither list"]
    assert sk.entry_cover(launch, other, collections.OrderedDict(sk.ENTRIES, vd_gone=sk.ENTRIES["vd_q_sample"]), sk.EXEMPT) == ["vd_gone: no vd_engine* entry of the header"]


def test_every_row_names_a_runner_and_what_is_compared():
    for name, row in sk.ENTRIES.items():
        assert row.run and row.outputs and "flags" in row.state, name
    assert {e for e, r in sk.ENTRIES.items() if r.run == "step"} == set(sk.SAMPLER_ENTRY.values())
    assert {sk.entry_of(c) for c in sk.STEP_ROWS} == set(sk.SAMPLER_ENTRY.values())          # every sampler's entry has a served row
    assert sk.FILLS == (0x00, 0x7F, 0xFF) and sk.HISTORIES == ("filled", "grown", "leftovers")
    B, T = sk.SHAPE
    assert sk.GROWN_SHAPE[0] > B and sk.GROWN_SHAPE[1] > T and sk.LONG_SHAPE[1] == 33
    for name in sk.EVALUATORS.values():
        assert name in _read(sk.HEADER)


def test_every_device_pointer_is_scratch_or_state_and_the_fill_fills_the_scratch():
    src = _read(sk.ENGINE)
    pointers, body = sk.engine_pointers(src), sk.fill_body(src)
    assert "ws" in pointers and "d_err" in pointers and "d_hid" in pointers and "d_lists" in pointers and len(pointers) >= 38
    assert "hipMemset" in body and "hipDeviceSynchronize" in body and "end_held" in body
    for word in ("grow(", "hipFree", "hipMalloc", "drop_window_graphs"):         # no address changes, no graph is dropped
        assert word not in body, word
    assert sk.buffer_cover(pointers, body, sk.SCRATCH, sk.STATE) == []
    # the comment above the entry is the classification: it names every pointer under one of the two headings
    head = src[src.index("// Test hook (include/vd_amd.h): every engine-owned SCRATCH"):src.index("int vd_scratch_fill(")]
    import re
    m_scratch, m_state = re.search(r"//\s+SCRATCH\s+ws\b", head), re.search(r"//\s+STATE\s+d_\w+", head)
    assert m_scratch and m_state and m_scratch.start() < m_state.start(), "the comment above vd_scratch_fill lost its two headings (SCRATCH ..., then STATE ...)"
    scratch_part, state_part = head[m_scratch.start():m_state.start()], head[m_state.start():]
    for n in sk.SCRATCH:
        assert re.search(rf"\b{n}\b", scratch_part) and not re.search(rf"\b{n}\b", state_part), n
    for n in sk.STATE:
        assert re.search(rf"\b{n}\b", state_part) and not re.search(rf"\b{n}\b", scratch_part), n
    # the mistakes the cover is there for
    drop = lambda names, n: tuple(x for x in names if x != n)                    # noqa: E731
    assert sk.buffer_cover(pointers, body, drop(sk.SCRATCH, "d_lin_r"), sk.STATE) == ["d_lin_r: a device pointer of struct vd_engine in neither list"]
    assert sk.buffer_cover(pointers, body, sk.SCRATCH, drop(sk.STATE, "d_win_hist")) == ["d_win_hist: a device pointer of struct vd_engine in neither list"]
    assert sk.buffer_cover(pointers, body, sk.SCRATCH + ("d_err",), sk.STATE) == ["d_err: in SCRATCH and in STATE", "d_err: scratch that vd_scratch_fill does not fill"]
    assert sk.buffer_cover(pointers, body.replace("e->d_part_x0", "nullptr"), sk.SCRATCH, sk.STATE) == ["d_part_x0: scratch that vd_scratch_fill does not fill"]
    assert sk.buffer_cover(pointers, body + " fill(e->d_cfg_zero, 4);", sk.SCRATCH, sk.STATE) == ["d_cfg_zero: state that vd_scratch_fill names"]
    grown = src.replace("    char* ws = nullptr; size_t ws_cap = 0;", "    char* ws = nullptr; size_t ws_cap = 0;\n    float* d_new_buf = nullptr;")
    assert sk.buffer_cover(sk.engine_pointers(grown), body, sk.SCRATCH, sk.STATE) == ["d_new_buf: a device pointer of struct vd_engine in neither list"]


def test_the_rows_served_again_cover_the_option_matrix():
    assert sk.option_cover(sk.STEP_ROWS, sk.WINDOW_ROWS) == []
    assert sk.DEEPEST in sm.stack_rows() and sk.DEEPEST in sk.STEP_ROWS and sk.DEEPEST in sm.matrix_rows()
    for r in sk.STEP_ROWS:
        assert r._replace(switch="none") == r and any(m._replace(switch="none") == r for m in sm.matrix_rows()), r     # rows of that file, not new ones
    for r in sk.WINDOW_ROWS:
        assert sm.status(r, "window") == "served", r
    assert len(sk.STEP_ROWS) <= 16 and len(set(sk.STEP_ROWS)) == len(sk.STEP_ROWS)
    # the mistakes the cover is there for: a value that only one row brings, the deepest stack, a switch, a refused row
    assert ("sampler", "unipc") in sk.option_cover([r for r in sk.STEP_ROWS if r.sampler != "unipc"], [w for w in sk.WINDOW_ROWS if w.sampler != "unipc"])
    assert ("stack", "deepest") in sk.option_cover([r for r in sk.STEP_ROWS if r != sk.DEEPEST], sk.WINDOW_ROWS)
    assert sk.option_cover(sk.STEP_ROWS, [w for w in sk.WINDOW_ROWS if w.switch != "suffix_skip"]) == [("switch", "suffix_skip")]
    assert ("restoration", "part_cell4") in sk.option_cover([r for r in sk.STEP_ROWS if r.restoration != "part_cell4"], sk.WINDOW_ROWS)
    refused = sm.Case("unipc", "eps", "off", "off", "known", "none")
    assert ("served", sm.case_id(refused)) in sk.option_cover(sk.STEP_ROWS + [refused], sk.WINDOW_ROWS)
    for axis in ("model", "guidance", "freeu"):
        for v in sm.AXES[axis]:
            assert (axis, v) in sk.option_cover([r for r in sk.STEP_ROWS if getattr(r, axis) != v], [w for w in sk.WINDOW_ROWS if getattr(w, axis) != v])
