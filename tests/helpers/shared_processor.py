"""One processor instance shared by four runner threads: each thread's output, and the counters at the end, must equal what one thread
gets from the same groups.  Pins the per-thread scratch and the per-call tally of the parse processors' Process()."""
import threading

from loongcollector_amd.processor import EventGroup


def _process(p, fixture):
    g = EventGroup(fixture)
    try:
        p.process(g)
        return (g.to_dict() or {}).get("events", [])
    finally:
        g.close()


def four_threads_equal_one_thread(make, groups):
    """make() -> a processor with process(EventGroup), counters() and close(); groups[t]: the fixture groups of thread t.
    -> (the single-thread outputs [t][g], the shared processor's counters)"""
    assert len(groups) == 4
    single = make()
    want = [[_process(single, g) for g in mine] for mine in groups]
    want_counters = single.counters()
    single.close()
    shared = make()
    got, errors = [None] * len(groups), []
    start = threading.Barrier(len(groups))

    def worker(t):
        try:
            start.wait()
            got[t] = [_process(shared, g) for g in groups[t]]
        except BaseException as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(len(groups))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    counters = shared.counters()
    shared.close()
    assert not errors, errors
    for t in range(len(groups)):
        assert got[t] == want[t], t
    assert counters == want_counters and counters["device_failed_events_total"] == 0
    return want, counters
