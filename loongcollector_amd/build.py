"""Build liblc_regex_gpu.so (host compilers + gfx950 kernels + C ABI) in-tree with hipcc.

    python -m loongcollector_amd.build          # or __graft_entry__.build()

The .so lands in loongcollector_amd/lib/ (git-ignored, but shipped to the GPU box by gpurun).
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "liblc_regex_gpu.so")
# the same library with the stand-in event model built in the REFERENCE's shape (csrc/event_model.hpp LC_REFERENCE_SHAPED_EVENT_MODEL:
# heap std::vector contents, no chunk pool, K x SetContentNoCopy + DelContent).  bench.py loads it in a process of its own for
# end_to_end.in_agent_reference_shape_MBps -- what an agent build's event model lets one runner thread do; never the default.
LIB_REFSHAPE = os.path.join(LIBDIR, "liblc_regex_gpu_refshape.so")

# the key-value splitter (include/kvsplit/lc_kvsplit.h): a library of its own beside LIB, linked against it; LIB's ABI does not grow
LIB_KV = os.path.join(LIBDIR, "liblc_kvsplit.so")
KV_SOURCES = ["kv_device.hip", "processor_split_key_value_gpu.cpp"]
# the CSV decoder (include/csv/lc_csv.h): the same again, a third library beside the two
LIB_CSV = os.path.join(LIBDIR, "liblc_csv.so")
CSV_SOURCES = ["csv_device.hip", "processor_csv_gpu.cpp"]
# the SLS encoder (include/sls/lc_sls.h): a fourth library beside the three
LIB_SLS = os.path.join(LIBDIR, "liblc_sls.so")
SLS_SOURCES = ["sls_device.hip", "sls_plan.cpp", "processor_sls_gpu.cpp"]
# the anchor processor (include/anchor/lc_anchor.h): a fifth library beside the four
LIB_ANCHOR = os.path.join(LIBDIR, "liblc_anchor.so")
ANCHOR_SOURCES = ["anchor_device.hip", "processor_anchor_gpu.cpp"]
# the LZ4 block writer (include/lz4/lc_lz4.h): a sixth library, linked against the main one and the SLS encoder's
LIB_LZ4 = os.path.join(LIBDIR, "liblc_lz4.so")
LZ4_SOURCES = ["lz4_device.hip"]
# the JSON-lines encoder (include/jsonl/lc_jsonl.h): a seventh library, linked against the main one
LIB_JSONL = os.path.join(LIBDIR, "liblc_jsonl.so")
JSONL_SOURCES = ["jsonl_device.hip", "jsonl_plan.cpp", "processor_jsonl_gpu.cpp"]
# the string-replace processor (include/strrep/lc_strrep.h): an eighth library, linked against the main one as the anchor processor's is
LIB_STRREP = os.path.join(LIBDIR, "liblc_strrep.so")
STRREP_SOURCES = ["strrep_device.hip", "processor_string_replace_gpu.cpp"]
# the field codecs (include/codec/lc_codec.h: base64 encode / decode, MD5): a ninth library, linked against the main one
LIB_CODEC = os.path.join(LIBDIR, "liblc_codec.so")
CODEC_SOURCES = ["codec_device.hip", "processor_codec_gpu.cpp"]
SIDE_SOURCES = KV_SOURCES + CSV_SOURCES + SLS_SOURCES + ANCHOR_SOURCES + LZ4_SOURCES + JSONL_SOURCES + STRREP_SOURCES + CODEC_SOURCES

SOURCES = ["regex_parse.cpp", "atomic_elide.cpp", "follow_nfa.cpp", "tdfa.cpp", "table_cache.cpp", "screen_dfa.cpp", "bt_program.cpp", "regex_handle.cpp", "gpu_runtime.hip", "grok_device.hip", "multiline_device.hip", "delim_device.hip", "strptime_program.cpp", "timestamp_device.hip", "json_device.hip", "apsara_device.hip", "clog_device.hip", "desens_device.hip", "prom_device.hip"]
OPTIONAL_SOURCES = ["event_model.cpp", "processor_parse_regex_gpu.cpp", "grok.cpp", "grok_literal_index.cpp", "processor_grok_gpu.cpp", "processor_filter_gpu.cpp", "processor_go_regex_gpu.cpp", "multiline_gpu.cpp", "multiline_events.cpp", "processor_pipeline_gpu.cpp", "processor_parse_delimiter_gpu.cpp", "processor_parse_timestamp_gpu.cpp", "processor_parse_json_gpu.cpp", "processor_parse_apsara_gpu.cpp", "processor_parse_container_log_gpu.cpp", "processor_desensitize_gpu.cpp", "processor_parse_prom_gpu.cpp", "c_processor_slot.cpp"]


# what the on-disk table cache's stamp is made of: the constructions, the structures they read and write, the cache's own format
TABLE_SHAPING_SOURCES = ["tdfa.cpp", "screen_dfa.cpp", "tdfa.hpp", "follow_nfa.hpp", "regex_ast.hpp", "table_cache.cpp"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def sources():
    out = [os.path.join(CSRC, s) for s in SOURCES]
    out += [os.path.join(CSRC, s) for s in OPTIONAL_SOURCES if os.path.exists(os.path.join(CSRC, s))]
    out += [os.path.join(CSRC, s) for s in SIDE_SOURCES]
    return out


def needs_build():
    if not os.path.exists(LIB) or not os.path.exists(LIB_KV) or not os.path.exists(LIB_CSV) or not os.path.exists(LIB_SLS) or \
            not os.path.exists(LIB_ANCHOR) or not os.path.exists(LIB_LZ4) or not os.path.exists(LIB_JSONL) or not os.path.exists(LIB_STRREP) or \
            not os.path.exists(LIB_CODEC):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    deps.append(os.path.join(HERE, "..", "include", "lc_regex_gpu.h"))
    deps.append(os.path.join(HERE, "..", "include", "lc_processor.h"))
    deps.append(os.path.join(HERE, "..", "include", "lc_grok.h"))
    deps.append(os.path.join(HERE, "..", "include", "lc_go_regex.h"))
    deps.append(os.path.join(HERE, "..", "include", "lc_multiline.h"))
    deps.append(os.path.join(HERE, "..", "include", "lc_delimiter.h"))
    deps.append(os.path.join(HERE, "..", "include", "lc_timestamp.h"))
    deps.append(os.path.join(HERE, "..", "include", "lc_json.h"))
    deps.append(os.path.join(HERE, "..", "include", "lc_apsara.h"))
    deps.append(os.path.join(HERE, "..", "include", "lc_container_log.h"))
    deps.append(os.path.join(HERE, "..", "include", "lc_desensitize.h"))
    deps.append(os.path.join(HERE, "..", "include", "lc_prom.h"))
    deps.append(os.path.join(HERE, "..", "include", "kvsplit", "lc_kvsplit.h"))
    deps.append(os.path.join(HERE, "..", "include", "csv", "lc_csv.h"))
    deps.append(os.path.join(HERE, "..", "include", "sls", "lc_sls.h"))
    deps.append(os.path.join(HERE, "..", "include", "anchor", "lc_anchor.h"))
    deps.append(os.path.join(HERE, "..", "include", "lz4", "lc_lz4.h"))
    deps.append(os.path.join(HERE, "..", "include", "jsonl", "lc_jsonl.h"))
    deps.append(os.path.join(HERE, "..", "include", "strrep", "lc_strrep.h"))
    deps.append(os.path.join(HERE, "..", "include", "codec", "lc_codec.h"))
    deps.append(os.path.join(HERE, "data", "grok_default_patterns.txt"))
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


CORPUS_SRC = os.path.join(HERE, "..", "tools", "corpus_gen.cpp")
CORPUS_LIB = os.path.join(LIBDIR, "libcorpus_gen.so")


def build_corpus_gen():
    """tools/corpus_gen.cpp (bench / test tooling: the headline corpus generated line by line from std::mt19937_64) -> lib/libcorpus_gen.so"""
    os.makedirs(LIBDIR, exist_ok=True)
    if os.path.exists(CORPUS_LIB) and os.path.getmtime(CORPUS_LIB) > os.path.getmtime(CORPUS_SRC):
        return CORPUS_LIB
    cxx = shutil.which("g++") or _hipcc()
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", CORPUS_LIB, CORPUS_SRC])
    return CORPUS_LIB


def build_native(force=False, verbose=False, force_sources=()):
    """force_sources: basenames of sources to recompile even if their objects look current (smoke() uses it to show a real
    gfx950 compile on the GPU box)."""
    if not force and not force_sources and not needs_build() and os.path.exists(LIB_REFSHAPE) and \
            os.path.getmtime(LIB_REFSHAPE) >= os.path.getmtime(LIB):
        return LIB
    os.makedirs(LIBDIR, exist_ok=True)
    objs = []
    objdir = os.path.join(LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)
    # the Grok default library (data/grok_default_patterns.txt) is compiled in as one raw string literal
    inc = os.path.join(objdir, "grok_defaults.inc")
    with open(os.path.join(HERE, "data", "grok_default_patterns.txt"), encoding="utf-8") as f:
        blob = 'R"GROKDATA(' + f.read() + ')GROKDATA"\n'
    if not os.path.exists(inc) or open(inc, encoding="utf-8").read() != blob:
        with open(inc, "w", encoding="utf-8") as f:
            f.write(blob)
    # the stamp of the on-disk table cache (csrc/table_cache.cpp): a hash of every source that shapes the compiled tables, so that an
    # edit of tdfa.cpp alone also invalidates what an older build of the library has written
    import hashlib
    hh = hashlib.sha256()
    for name in TABLE_SHAPING_SOURCES:
        with open(os.path.join(CSRC, name), "rb") as f:
            hh.update(name.encode() + b"\0" + f.read() + b"\0")
    stamp = '"lc-tables-%s"\n' % hh.hexdigest()[:32]
    stamp_inc = os.path.join(objdir, "table_sources_stamp.inc")
    if not os.path.exists(stamp_inc) or open(stamp_inc).read() != stamp:
        with open(stamp_inc, "w") as f:
            f.write(stamp)
    common = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-result", "-I", os.path.join(HERE, "..", "include"),
              "-I", CSRC, "-I", objdir] + os.environ.get("LC_EXTRA_CXXFLAGS", "").split()
    procs = []
    for src in sources():
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        objs.append(obj)
        if (not force and os.path.basename(src) not in force_sources and os.path.exists(obj) and os.path.getmtime(obj) > os.path.getmtime(src)
                and (os.path.basename(src) != "table_cache.cpp" or os.path.getmtime(obj) > os.path.getmtime(stamp_inc))
                and all(os.path.getmtime(obj) > os.path.getmtime(os.path.join(CSRC, h))
                        for h in os.listdir(CSRC) if h.endswith((".h", ".hpp")))):
            continue
        cmd = [_hipcc(), "--offload-arch=gfx950"] + common
        if src.endswith(".hip"):
            cmd += ["-x", "hip"]
        cmd += ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (src, out.decode()))
        if verbose and out:
            print(out.decode(), file=sys.stderr)
    kv_objs = [o for o in objs if os.path.basename(o)[:-2] in KV_SOURCES]
    csv_objs = [o for o in objs if os.path.basename(o)[:-2] in CSV_SOURCES]
    sls_objs = [o for o in objs if os.path.basename(o)[:-2] in SLS_SOURCES]
    anchor_objs = [o for o in objs if os.path.basename(o)[:-2] in ANCHOR_SOURCES]
    lz4_objs = [o for o in objs if os.path.basename(o)[:-2] in LZ4_SOURCES]
    jsonl_objs = [o for o in objs if os.path.basename(o)[:-2] in JSONL_SOURCES]
    strrep_objs = [o for o in objs if os.path.basename(o)[:-2] in STRREP_SOURCES]
    codec_objs = [o for o in objs if os.path.basename(o)[:-2] in CODEC_SOURCES]
    objs = [o for o in objs if o not in kv_objs and o not in csv_objs and o not in sls_objs and o not in anchor_objs and o not in lz4_objs
            and o not in jsonl_objs and o not in strrep_objs and o not in codec_objs]
    # (the SONAME: liblc_kvsplit.so names this library as needed, and a process that has it loaded already -- from a file a later build has
    # replaced -- must get THAT copy, not a second one)
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-soname,liblc_regex_gpu.so", "-o", LIB] + objs
    subprocess.check_call(cmd)
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_KV] + kv_objs +
                          ["-L" + LIBDIR, "-llc_regex_gpu", "-Wl,-rpath,$ORIGIN"])
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_CSV] + csv_objs +
                          ["-L" + LIBDIR, "-llc_regex_gpu", "-Wl,-rpath,$ORIGIN"])
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_SLS] + sls_objs +
                          ["-L" + LIBDIR, "-llc_regex_gpu", "-Wl,-rpath,$ORIGIN"])
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_ANCHOR] + anchor_objs +
                          ["-L" + LIBDIR, "-llc_regex_gpu", "-Wl,-rpath,$ORIGIN"])
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_LZ4] + lz4_objs +
                          ["-L" + LIBDIR, "-llc_sls", "-llc_regex_gpu", "-Wl,-rpath,$ORIGIN"])
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_JSONL] + jsonl_objs +
                          ["-L" + LIBDIR, "-llc_regex_gpu", "-Wl,-rpath,$ORIGIN"])
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_STRREP] + strrep_objs +
                          ["-L" + LIBDIR, "-llc_regex_gpu", "-Wl,-rpath,$ORIGIN"])
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_CODEC] + codec_objs +
                          ["-L" + LIBDIR, "-llc_regex_gpu", "-Wl,-rpath,$ORIGIN"])
    # the reference-shaped variant: only the host translation units that see the event model are compiled again (with the switch);
    # the regex compilers and every gfx950 object are the ones just linked above
    shape_objs, procs = [], []
    for src, obj in zip([s for s in sources() if os.path.basename(s) not in SIDE_SOURCES], objs):
        base = os.path.basename(src)
        if base not in OPTIONAL_SOURCES:
            shape_objs.append(obj)
            continue
        sobj = os.path.join(objdir, base + ".refshape.o")
        shape_objs.append(sobj)
        if (not force and os.path.exists(sobj) and os.path.getmtime(sobj) > os.path.getmtime(src)
                and all(os.path.getmtime(sobj) > os.path.getmtime(os.path.join(CSRC, h))
                        for h in os.listdir(CSRC) if h.endswith((".h", ".hpp")))):
            continue
        cmd = [_hipcc(), "--offload-arch=gfx950"] + common + ["-DLC_REFERENCE_SHAPED_EVENT_MODEL", "-c", src, "-o", sobj]
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed for %s (reference-shaped variant):\n%s" % (src, out.decode()))
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_REFSHAPE] + shape_objs)
    return LIB


if __name__ == "__main__":
    print(build_native(force="--force" in sys.argv, verbose=True))
