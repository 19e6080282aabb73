"""A model of the reference's plugins/processor/anchor/anchor.go on `bytes`: Init :74-99, ProcessLog :112-129 and the string half of
ProcessAnchor :172-199, statement by statement.  `bytes.find` is Go's strings.Index (the first occurrence, 0 for an empty needle, -1 for
none); CPython's search shares nothing with csrc/anchor_vm.hpp, so this is an independent reference -- the reference of every anchor
test.  A json anchor is refused, as include/anchor/lc_anchor.h DEFINES it."""

NO_START, NO_STOP = -1, -2
ALARM_NO_KEY, ALARM_NO_START, ALARM_NO_STOP, ALARM_TRIP_FAILED = 1, 2, 3, 4
MAX_ANCHORS, MAX_NEEDLE = 16, 32


class Refused(ValueError):
    pass


def _b(x):
    return x.encode("utf-8") if isinstance(x, str) else bytes(x)


def init(config):
    """the Go struct with every absent field at its zero value (there are no defaults), strings as bytes"""
    anchors = []
    for i, a in enumerate(config.get("Anchors", [])):
        if a.get("FieldType", "") == "json":  # :80 -- DEFINED: refused
            raise Refused("anchor %d has FieldType json" % i)
        anchors.append({"Start": _b(a.get("Start", "")), "Stop": _b(a.get("Stop", "")), "FieldName": _b(a.get("FieldName", ""))})  # :78, :91-92
        if len(anchors[-1]["Start"]) > MAX_NEEDLE or len(anchors[-1]["Stop"]) > MAX_NEEDLE:
            raise Refused("anchor %d: a needle above %d bytes" % (i, MAX_NEEDLE))
    if len(anchors) > MAX_ANCHORS:
        raise Refused("%d anchors" % len(anchors))
    return {"Anchors": anchors, "NoKeyError": bool(config.get("NoKeyError", False)), "NoAnchorError": bool(config.get("NoAnchorError", False)),
            "SourceKey": _b(config.get("SourceKey", "")), "KeepSource": bool(config.get("KeepSource", False))}


def cut_string(val, max_len=1024):
    """util.CutString"""
    return val if len(val) < max_len else val[0:max_len]


def locate_one(anchor, val):
    """:175-195 for one anchor -> (b, e), (NO_START, -1) or (NO_STOP, -1)"""
    start_index = val.find(anchor["Start"])          # :175
    if start_index < 0:                              # :176
        return (NO_START, -1)
    start_index += len(anchor["Start"])              # :182
    stop_index = val[start_index:].find(anchor["Stop"])  # :183
    if stop_index < 0:                               # :184
        return (NO_STOP, -1)
    if len(anchor["Stop"]) == 0:                     # :190
        stop_index = len(val)
    else:
        stop_index += start_index                    # :193
    return (start_index, stop_index)


def locate(config, val):
    """-> one (b, e) per anchor, as the ABI reports them"""
    return [locate_one(a, _b(val)) for a in init(config)["Anchors"]]


def process_anchor(c, contents, val, alarms):
    """ProcessAnchor :172-199 (string anchors)"""
    for anchor in c["Anchors"]:
        b, e = locate_one(anchor, val)
        if b == NO_START:
            if c["NoAnchorError"]:  # :177-179
                alarms.append((ALARM_NO_START, b"anchor no start:" + anchor["Start"] + b"\tcontent:" + cut_string(val) + b"\t"))
            continue
        if b == NO_STOP:
            if c["NoAnchorError"]:  # :185-187
                alarms.append((ALARM_NO_STOP, b"anchor no stop:" + anchor["Stop"] + b"\tcontent:" + cut_string(val) + b"\t"))
            continue
        contents.append([anchor["FieldName"], val[b:e]])  # :199


def process_log(config, contents):
    """ProcessLog :112-129.  contents: [[key, value], ...] -> (new contents, [(kind, text)], the pairs-per-log metric of :128)"""
    c = init(config)
    contents = [[_b(k), _b(v)] for k, v in contents]
    begin_len = len(contents)                                      # :113
    alarms = []
    find_key = False
    for i, (key, value) in enumerate(list(contents)):              # :115
        if len(c["SourceKey"]) == 0 or c["SourceKey"] == key:      # :116
            find_key = True
            if not c["KeepSource"]:                                # :118-120
                del contents[i]
            process_anchor(c, contents, value, alarms)             # :121
            break
    if not find_key and c["NoKeyError"]:                           # :125-127
        alarms.append((ALARM_NO_KEY, b"anchor cannot find key:" + c["SourceKey"] + b"\t"))
    return contents, alarms, len(contents) - begin_len + 1         # :128
