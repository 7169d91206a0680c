"""The backward's ONE predicate for "the window-attention backward runs" against the condition the captured backward used before it was shared
(`_reads_frames_embed`: whether a replayed graph must refresh its static copy of frames_embed), over every combination of the flags.  No GPU."""
import itertools
from types import SimpleNamespace

from hicom_amd import autograd as hag

MODES = (None, "off", "direct", "coarse", "fine")
FLAGS = tuple(itertools.product((False, True), repeat=8))      # adapt_q, adapt_k, adapt_v, adapt_guide, clip, want_fe, want_guide, have_ctx


def _proj(use_guide, adapt_q, adapt_k, adapt_v, adapt_guide, clip):
    lc = SimpleNamespace(use_guide=use_guide, adapt_q=adapt_q, adapt_k=adapt_k, adapt_v=adapt_v, adapt_guide=adapt_guide)
    return SimpleNamespace(local_compressor=lc, local_logit=(2.0, -3.0) if clip else None)


def test_reads_frames_embed_equals_the_former_expression_for_every_flag_combination():
    checked = 0
    for use_guide in MODES:
        for adapt_q, adapt_k, adapt_v, adapt_guide, clip, want_fe, want_guide, have_ctx in FLAGS:
            proj = _proj(use_guide, adapt_q, adapt_k, adapt_v, adapt_guide, clip)
            local_logit = proj.local_logit
            mode = use_guide if use_guide not in (None, "off") else None
            query_params = mode in ("coarse", "fine") or adapt_q or adapt_guide
            want = (not have_ctx) or want_fe or adapt_k or adapt_v or query_params or (want_guide and mode is not None) or local_logit is not None
            got = hag._reads_frames_embed(proj, want_fe, want_guide, have_ctx)
            assert isinstance(got, bool) and got == bool(want), (use_guide, adapt_q, adapt_k, adapt_v, adapt_guide, clip, want_fe, want_guide, have_ctx)
            checked += 1
    assert checked == 5 * 256


def test_reads_frames_embed_is_false_without_a_local_stage():
    for clip, want_fe, want_guide, have_ctx in itertools.product((False, True), repeat=4):
        proj = SimpleNamespace(local_compressor=None, local_logit=(2.0, -3.0) if clip else None)
        assert hag._reads_frames_embed(proj, want_fe, want_guide, have_ctx) is False


def test_window_backward_predicate_is_the_frames_embed_predicate_plus_the_frames_feature_request():
    """With the forward's contexts kept, frames_embed is read exactly when the window backward runs without a d frames_feature request (the
    captured backward never carries one); asking for d frames_feature always runs it."""
    for use_guide in MODES:
        for adapt_q, adapt_k, adapt_v, adapt_guide, clip, want_fe, want_guide, _ in FLAGS[::2]:
            proj = _proj(use_guide, adapt_q, adapt_k, adapt_v, adapt_guide, clip)
            runs = hag._window_backward_runs(proj.local_compressor, want_fe, want_guide, proj.local_logit, False)
            assert runs == hag._reads_frames_embed(proj, want_fe, want_guide, True)
            assert hag._window_backward_runs(proj.local_compressor, want_fe, want_guide, proj.local_logit, True) is True
