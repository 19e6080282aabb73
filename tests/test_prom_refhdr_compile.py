"""processor_prom_parse_metric_gpu type-checked against the reference's OWN headers, as tests/test_refhdr_compile.py does for the other
processors: with -DLC_USE_REFERENCE_HEADERS csrc/processor_parse_prom_gpu.cpp sees core/models/MetricEvent.h, RawEvent.h and
PipelineEventGroup.h instead of the stand-in (csrc/event_model.hpp), so every call it makes on MetricEvent -- SetNameNoCopy,
SetValue<UntypedSingleValue>, SetTag, SetTagNoCopy, SetTimestamp, CreateMetricEvent, the three-argument emplace_back of the events
container, EventGroupMetaKey::PROMETHEUS_SCRAPE_TIMESTAMP_MILLISEC -- exists there with those argument types.  A second translation
unit makes the calls the tests' double and the fixture accessors make on the stand-in (GetName, GetValue, TagsBegin / TagsEnd /
TagsSize, Is<MetricEvent>), against the reference's class.

/root/reference does not exist on the GPU box: the tests are skipped there."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/core"
CSRC = os.path.join(ROOT, "loongcollector_amd", "csrc")

pytestmark = pytest.mark.skipif(not os.path.isdir(REF) or shutil.which("g++") is None, reason="needs the reference tree (/root/reference) and g++")

FLAGS = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-DLC_USE_REFERENCE_HEADERS", "-I", os.path.join(ROOT, "tests", "refhdr"), "-I", REF,
         "-I", os.path.join(REF, "config"), "-I", os.path.join(ROOT, "include"), "-I", CSRC]

READERS = r"""
#include "processor_parse_prom_gpu.hpp"
#include "models/MetricEvent.h"
#include "models/RawEvent.h"
uint64_t readBack(logtail::PipelineEventGroup& group) {
    uint64_t sum = 0;
    for (const logtail::PipelineEventPtr& e : group.GetEvents()) {
        if (!e.Is<logtail::MetricEvent>()) continue;
        const logtail::MetricEvent& m = e.Cast<logtail::MetricEvent>();
        sum += m.GetName().size() + m.TagsSize();
        if (m.Is<logtail::UntypedSingleValue>()) sum += uint64_t(m.GetValue<logtail::UntypedSingleValue>()->mValue);
        for (auto it = m.TagsBegin(); it != m.TagsEnd(); ++it) sum += it->first.size() + it->second.size();
        sum += uint64_t(e->GetTimestamp()) + (e->GetTimestampNanosecond() ? *e->GetTimestampNanosecond() : 0);
    }
    group.AddRawEvent()->SetContentNoCopy(logtail::StringView("m 1", 3));
    group.SetMetadata(logtail::EventGroupMetaKey::PROMETHEUS_SCRAPE_TIMESTAMP_MILLISEC, std::string("1"));
    return sum;
}
"""


def test_processor_type_checks_against_the_reference_headers():
    r = subprocess.run(FLAGS + [os.path.join(CSRC, "processor_parse_prom_gpu.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


def test_the_readers_calls_exist_on_the_references_metric_event(tmp_path):
    probe = tmp_path / "prom_readers_probe.cpp"
    probe.write_text(READERS)
    r = subprocess.run(FLAGS + [str(probe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


def test_the_reference_headers_are_really_the_ones_parsed(tmp_path):
    """guard against a silently ignored switch: the reference's MetricEvent has DelTag, the stand-in does not -- with the switch a call
    compiles, without it the same translation unit must fail"""
    probe = tmp_path / "prom_deltag_probe.cpp"
    probe.write_text('#include "processor_parse_prom_gpu.hpp"\n#ifdef LC_USE_REFERENCE_HEADERS\n#include "models/MetricEvent.h"\n#endif\n'
                     'void probe(logtail::MetricEvent& e) { e.DelTag(logtail::StringView("a", 1)); }\n')
    with_switch = subprocess.run(FLAGS + [str(probe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert with_switch.returncode == 0, with_switch.stdout[-2000:]
    without = subprocess.run([f for f in FLAGS if f != "-DLC_USE_REFERENCE_HEADERS"] + [str(probe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert without.returncode != 0 and "DelTag" in without.stdout, without.stdout[-2000:]
