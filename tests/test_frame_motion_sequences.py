"""The inputs of tests/test_gpu_frame_motion.py, checked without a GPU: the CPU oracle renders sequence (a) of
frame_motion_util - the hand-built wall and two cards on the upload path - at the two shapes whose conditions the GPU test
asserts, and the model's middle frame has MOVED pixels with history, UNMOVED pixels and pixels without history, at 260 x 2 on
both sides of the block seam.  The conditions then test the inputs, not the kernel."""
import numpy as np
import pytest

import frame_denoise_util as fu
import frame_motion_util as mu
import frame_temporal_util as tu

D = fu.CORNELL
T = dict(tu.CORNELL, flags=mu.MOTION | mu.SAME_INSTANCE)


@pytest.mark.parametrize("width,height", ((70, 37), (260, 2)))
def test_the_oracles_frames_of_sequence_a_meet_the_conditions(W, oracle_lib, width, height):
    o = oracle_lib.OracleRenderer()
    o.buildPipeline(4, 1)
    st = mu.History()
    for k in range(3):
        b, ids = mu.sequence_a(k, width, height)
        mu.upload_frame(W, o, b, ids, width, height, k == 0)
        o.compute(k + 1)
        fr = fu.frame_of(o.readAccum(), o.readGBuffer(), o.readUniforms())
        _, integ, acc, c = mu.call(fr, mu.scene_of(b, ids), D, T, st)
        if k == 1:
            mu.sequence_conditions(c, st.n(), st.guide, width, height)
        if k >= 1:
            # the ids follow the cards through the reorders: card A (stable id 1) is MOVED wherever it is seen, the rest UNMOVED
            s, sid = mu.status(c), fu.words(c[..., 7])
            surf = fu.words(st.guide[..., 7]) != 0
            assert (s[surf & (sid == 1)] == mu.MOVED).all() and (s[surf & (sid != 1)] == mu.UNMOVED).all(), k
            assert (sid[surf] < 3).all() and (sid[~surf] == mu.NO_ID).all()
    assert st.frames == 3 and st.n().max() == 3
