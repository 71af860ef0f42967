"""The one reset of the session-wide Engine the GPU tests share: every module starts, and leaves, in the state it would
have in a process of its own, whichever module ran before it and however that one ended."""


def reset(engine):
    """Every option at the default of the library's table (Engine.reset_options: the environment overrides of
    psa_create are ignored), the product K1 selector, no atom weights, no segments."""
    from psa_amd import _hip
    engine.reset_options()
    engine.set_k1(_hip.K1_AUTO)
    engine.set_atom_weights(None)
    engine.set_segments(None)
