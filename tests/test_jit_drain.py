"""dq_pred_jit_drain joins the background predicate compiles; the package registers it to run when the interpreter
exits.  With nothing running it returns at once, any number of times."""


def test_drain_with_nothing_running():
    from deequ_amd import _lib as L

    assert "dq_pred_jit_drain" in L.EXPORTED
    L.lib.dq_pred_jit_drain()
    L.lib.dq_pred_jit_drain()
