"""Host: the option matrix of tests/step_matrix_cases.py covers what it says it covers -- every pair of axis values, a status for every
row at every entry, refusal fragments that are text of the sources, every axis value served somewhere, and no row left out."""
import os

import step_matrix_cases as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video-diffusion_amd")
SOURCES = [os.path.join(PKG, "csrc", "engine.hip"), os.path.join(PKG, "gaussian_diffusion.py"), os.path.join(PKG, "executor.py")]


def test_every_pair_of_values_from_two_axes_is_in_a_row():
    rows = sm.pairwise_rows()
    covered = set().union(*(sm.pairs_of(r) for r in rows))
    missing = [p for p in sm.all_pairs() if p not in covered]
    print(f"{len(rows)} pairwise rows cover {len(sm.all_pairs())} pairs; {len(sm.stack_rows())} stack rows, {len(sm.matrix_rows())} in all")
    assert not missing, missing[:5]
    assert 56 <= len(rows) <= 80                                                 # 56 = 8 x 7, the two longest axes: no set is smaller
    assert len(set(rows)) == len(rows) and rows == sm.pairwise_rows()           # no row twice; the same set on every call
    other = sm.pairwise_rows(seed=1)
    assert other != rows and not [p for p in sm.all_pairs() if p not in set().union(*(sm.pairs_of(r) for r in other))]
    for r in rows:
        assert all(getattr(r, a) in vals for a, vals in sm.AXES.items())


def test_the_stack_rows_are_the_deep_stack():
    rows = sm.stack_rows()
    assert len(rows) == len(set(rows)) == 2 * (6 * 2 + 3)                        # 6 samplers walk down, 3 of them draw noise
    for r in rows:
        assert (r.guidance, r.freeu, r.switch) == ("w2_phi0.7_p0.9", "adaptive", "none") and not sm.walks_up(r)
        assert r.restoration in ("linear", "known", "part_linear") and (r.restoration != "part_linear" or sm.draws_noise(r))
    assert sm.status(sm.Case("unipc", "eps", "w2_phi0.7_p0.9", "adaptive", "known", "none"), "step")[0] == "refused"
    assert all(r in sm.matrix_rows() for r in rows) and len(set(sm.matrix_rows())) == len(sm.matrix_rows())


def test_status_is_total_and_accounts_for_every_row():
    counts = {e: {"served": 0, "refused": 0, "ignored": 0} for e in sm.ENTRIES}
    for r in sm.matrix_rows():
        for e in sm.ENTRIES:
            s = sm.status(r, e)
            kind = s if isinstance(s, str) else s[0]
            assert kind in counts[e], (r, e, s)                                  # three statuses, nothing skipped and nothing expected to fail
            if kind == "refused":
                assert len(s) == 2 and s[1] and all(isinstance(p, str) and p for p in ((s[1],) if isinstance(s[1], str) else s[1])), (r, e, s)
            else:
                assert s == kind
            counts[e][kind] += 1
    for e in sm.ENTRIES:
        print(e, counts[e])
        assert sum(counts[e].values()) == len(sm.matrix_rows())
    assert counts["step"]["ignored"] == 0 and counts["window"]["ignored"] == 0 and counts["p_mean_variance"]["refused"] == 0


def test_every_refusal_fragment_is_text_of_the_sources():
    text = [open(p, encoding="utf-8").read() for p in SOURCES]
    seen = set()
    for r in sm.matrix_rows():
        for e in sm.ENTRIES:
            s = sm.status(r, e)
            if not isinstance(s, str):
                seen.add(s[1])
    assert len(seen) >= 10
    for frag in sorted(seen, key=str):
        for piece in ((frag,) if isinstance(frag, str) else frag):
            assert any(piece in t for t in text), (frag, piece)


def test_fragment_in_reads_the_pieces_in_order():
    msg = "ddim_sample at eta = 0 inside steering_scope is not served: the step draws no noise"
    assert sm.fragment_in(("ddim_sample", " at eta = 0", " inside steering_scope is not served"), msg)
    assert not sm.fragment_in((" at eta = 0", "ddim_sample"), msg) and not sm.fragment_in("p_sample", msg)
    assert sm.fragment_in("steering_scope", msg)


def test_every_axis_value_is_served_in_some_row():
    """At the step entry for the sampler, guidance, FreeU and restoration axes (the window column refuses most rows that carry a window
    switch), and every switch and both models at the window entry."""
    rows = sm.matrix_rows()
    for axis in ("sampler", "guidance", "freeu", "restoration", "model"):
        for v in sm.AXES[axis]:
            assert any(getattr(r, axis) == v and sm.status(r, "step") == "served" for r in rows), (axis, v)
    for axis in ("sampler", "model", "guidance", "freeu", "restoration", "switch"):
        for v in sm.AXES[axis]:
            assert any(getattr(r, axis) == v and sm.status(r, "window") == "served" for r in rows), (axis, v)
    assert (len(sm.AXES["sampler"]), len(sm.AXES["guidance"]), len(sm.AXES["freeu"]), len(sm.AXES["restoration"])) == (7, 5, 3, 8)


def test_the_rules_against_the_docstrings_examples():
    """A few combinations whose status the docstrings state in so many words."""
    C = sm.Case
    assert sm.status(C("p_sample", "eps", "w2", "on", "known", "none"), "p_mean_variance") == "ignored"          # known_region_scope: not honoured by p_mean_variance
    assert sm.status(C("unipc", "eps", "off", "off", "meas_s2_colour", "none"), "step") == "served"               # measurement_scope: ... and unipc_sample
    assert sm.status(C("dpmpp_2m_sde", "xstart", "w2_phi0.7_p0.9", "adaptive", "part_linear", "none"), "window") == "served"
    assert sm.status(C("ddim_eta0", "eps", "off", "off", "part_cell4", "none"), "step")[0] == "refused"           # steering_scope: ddim_sample at eta = 0
    assert sm.status(C("p_sample", "eps", "off", "on", "none", "prefix_cache"), "window")[0] == "refused"         # freeu_scope: a WindowExecutor with prefix_cache
    assert sm.status(C("p_sample", "eps", "off", "off", "none", "suffix_skip"), "window") == "served"
    assert sm.batch(C("p_sample", "eps", "off", "off", "part_blur5", "none")) == 4 and sm.batch(C("p_sample", "eps", "off", "off", "known", "none")) == 2


def test_every_key_axis_was_the_differing_one():
    """The keying of test_gpu_step_matrix.test_row cycles over the guidance, FreeU and restoration axes: each is the differing axis of some served row."""
    differing = set()
    for index, case in enumerate(sm.matrix_rows()):
        partner = sm.keying_partner(case, index) if sm.status(case, "window") == "served" else None
        if partner is not None:
            differing |= {a for a in sm.KEY_AXES if getattr(partner, a) != getattr(case, a)}
    assert differing == set(sm.KEY_AXES)
