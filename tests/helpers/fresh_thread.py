"""run(fn): fn() on a thread of its own, which starts with an empty lc_last_error() and no device resources; returns what fn returned or
raises what it raised."""
import threading


def run(fn):
    box = {}

    def body():
        try:
            box["value"] = fn()
        except BaseException as e:      # noqa: BLE001
            box["error"] = e

    t = threading.Thread(target=body)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]
