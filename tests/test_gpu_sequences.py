"""Random call sequences against the CPU model of a context (tests/context_model.py).

Every committed seed's op list (tests/sequence_ops.py) runs on a PathTracer and on the
model; whatever an op returns -- statistics, query records, a read image, a refusal's code
-- and the images at the checkpoints must agree at 0 ulp.  Two variants: "pipelined" reads
nothing back between ops but what an op itself returns and compares the accumulation, the
moments and the last guide, denoised and display images every 8 to 12 ops and at the end;
"synchronised" compares them after every op.  Where only the pipelined variant fails, the
defect is one of ordering between the context's streams; where both fail, a cache outlived
what it was made for.  Frames are 40x30 and smaller; a test takes a few seconds."""
import pytest

import sequence_ops as Q
from pnraytracing_amd.tracer import PathTracer

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", ["pipelined", "synchronised"])
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_sequence_equals_the_model(seed, variant):
    w = Q.world_of(seed)
    ops = Q.sequence(seed)
    ref, _ = Q.model_run(seed)
    at = range(len(ops)) if variant == "synchronised" else Q.checkpoints(seed, len(ops))
    keep = []
    with PathTracer(0) as pt:
        w.start(pt, Q.starts_with_moments(seed))
        for k, op in enumerate(ops):
            where = f"seed {seed} ({variant}) op {k} {op!r}"
            want, images = ref[k]
            d = Q.difference(Q.apply(op, pt, w, keep), want)
            assert d is None, f"{where}: what the call returned: {d}"
            if k in at:
                for name, img in Q.snapshot(pt, tuple(images)).items():
                    d = Q.difference(img, images[name])
                    assert d is None, f"{where}: {name} image: {d}"
                del keep[:]                  # (the reads waited for every call that used the ray buffers)
