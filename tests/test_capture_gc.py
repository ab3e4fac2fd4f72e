"""mi355.no_gc_in_capture, the guard around every graph capture of the package: dead reference cycles (a dropped DAStep with its
graphs is one) are collected on entry, the cyclic collector stays off inside and comes back as it was."""
import gc
import weakref


class _Node:
    pass


def test_guard_collects_on_entry_and_keeps_the_collector_off_inside():
    import mi355
    assert gc.isenabled()
    gc.disable()
    try:
        a, b = _Node(), _Node()
        a.other, b.other = b, a
        w = weakref.ref(a)
        del a, b
        assert w() is not None                       # a cycle: only the collector frees it
        gc.enable()
        with mi355.no_gc_in_capture():
            assert w() is None and not gc.isenabled()
            c, d = _Node(), _Node()
            c.other, d.other = d, c
            w2 = weakref.ref(c)
            del c, d
            junk = [[i] for i in range(5000)]        # enough allocations for several automatic collections, were they on
            assert w2() is not None and len(junk) == 5000
        assert gc.isenabled()
        gc.disable()
        with mi355.no_gc_in_capture():
            assert not gc.isenabled()
        assert not gc.isenabled()                    # it was off before: it stays off
    finally:
        gc.enable()


def test_the_capture_sites_use_the_guard():
    import inspect
    import mi355.da_step
    import mi355.infer
    assert 'no_gc_in_capture()' in inspect.getsource(mi355.da_step.DAStep.capture)
    assert 'no_gc_in_capture()' in inspect.getsource(mi355.infer.GraphedForward.__call__)
