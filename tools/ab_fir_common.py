"""What tools/ab_fir.py, tools/ab_fir_real.py and tools/ab_large_fir.py share: the event timing of one call, the round robin over the
timed entries, and a device pointer as a torch tensor.  torch is imported on first use, so a tool may run a path of its own without it."""


def timed(fn, stream):
    """the milliseconds of fn() between two events on `stream`"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def round_robin(fns, reps, stream=None, alternate=False):
    """{name: the sorted times of `reps` calls}, every fn warmed up twice first.  With a stream the fns are timed here; without one every
    fn returns its own milliseconds.  alternate: forwards and backwards in turn -- what ran just before an entry (and left its bytes in
    the caches) changes with the direction, so two builds of the same kernel are not timed in one fixed order"""
    import torch
    ts = {n: [] for n in fns}
    for fn in fns.values():
        fn(), fn()
    torch.cuda.synchronize()
    for rep in range(reps):
        items = list(fns.items())
        for name, fn in (reversed(items) if alternate and rep % 2 else items):
            ts[name].append(fn() if stream is None else timed(fn, stream))
    return {n: sorted(v) for n, v in ts.items()}


class _Raw:
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3}


def as_tensor(ptr, shape, typestr="<c8"):
    """a device pointer as a torch tensor (no copy); typestr: "<c8" complex64, "<f4" float32"""
    import torch
    return torch.as_tensor(_Raw(ptr, tuple(shape), typestr), device="cuda")
