"""CPU-side checks of the stack-limit scenes of tests/test_gpu_limits.py (no
GPU): the chains really drive a traversal stack to the library's limit, and
the oracle renders them like the builder's own tree."""
import test_gpu_limits as L


def test_chain_model_reaches_the_stack_limit():
    """The float64 model: for each row order and chain kind, in at least one of
    its split axes, some camera ray holds stack_limit - 3 deferred siblings at
    once (measured: stack_limit - 2 = 62, on both axes for the leaf-left chain
    and on axis 0 for the interior-left one; 1 on its axis 2, where every camera
    ray has dir.z < 0 and the leaf is always the near child)."""
    D = L.PT_STACK - 2
    assert L.FAN_ROT > 0 and D < L.N_FAN
    for rot in (0, L.FAN_ROT):
        for kind in ("leafleft", "interiorleft"):
            peaks = {}
            for axis in (0, 2):
                cfg = L.chain_config(kind, axis, rot, D)
                pk = L.peak_deferred(cfg.packed.nodes, *L.primary_rays(cfg))
                peaks[axis] = int(pk.max())
                print(f"{cfg.name}: peak {pk.max()} deferred siblings, {int((pk >= D - 6).sum())} of {len(pk)} "
                      f"camera rays hold >= {D - 6}")
            assert max(peaks.values()) >= D - 1, (kind, rot, peaks)


def test_chain_oracle_equals_builder_tree():
    """The eight depth-(stack_limit - 2) chains (two kinds, two axes, two row
    orders) over the permuted rows render the builder tree's image (no stack
    overflow: oracle_render asserts it)."""
    assert len(L.CHAINS) == 8
    for ch in L.CHAINS:
        cfg = L.chain_config(*ch)
        L.assert_bitwise(L.oracle_render(cfg, 0, 2), L.fan_reference(), f"oracle: {cfg.name} vs builder tree")
