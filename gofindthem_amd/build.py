"""In-tree build of the HIP/C++ pieces for gfx950 (no cmake needed: a handful of hipcc/g++ invocations).

    python -m gofindthem_amd.build          # builds libgft.so (product) and libgfworkload.so (bench utility)

hipcc cross-compiles gfx950 code objects without a GPU, so this runs in the CPU-only container; the built
.so files are git-ignored but travel to the GPU box with the repository snapshot.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libgft.so")
ARCH = "gfx950"

# the product library carries the two production scan kernels (scan5, scan3) and the DFA kernel (an independent algorithm,
# the cross-check); GFT_EXTRA_KERNELS=1 adds the earlier suffix-window kernels scan2 / scan4 (tools/ studies, the opt-in
# cross-check job of tests/test_gpu_parity.py)
EXTRA = os.environ.get("GFT_EXTRA_KERNELS", "0") == "1"
HIP_SOURCES = ["gft_kernels.hip", "gft_solve.hip", "gft_scan3.hip", "gft_scan5.hip", "gft_compact.hip", "gft_tolower.hip", "gft_rules.hip", "gft_json.hip", "gft_tags.hip", "gft_result.hip", "gft_tagdoc.hip", "gft_split.hip", "gft_select.hip", "gft_context.hip", "gft_route.hip", "gft_spans.hip", "gft_lowermap.hip", "gft_excerpt.hip", "gft_mark.hip", "gft_replace.hip", "gft_stats.hip", "gft_words.hip", "gft_rank.hip"] + (["gft_scan2.hip", "gft_scan4.hip"] if EXTRA else [])
STAMP = os.path.join(CSRC, ".build_flags")
CXX_SOURCES = ["gft_api.cpp", "gft_pipeline.cpp", "gft_process.cpp", "gft_staging.cpp", "gft_lower_api.cpp", "gft_rules_api.cpp", "gft_tags_api.cpp", "gft_result_api.cpp", "gft_tagdoc_api.cpp", "gft_json_api.cpp", "gft_split_api.cpp", "split_host.cpp", "gft_select_api.cpp", "select_host.cpp", "gft_context_api.cpp", "context_host.cpp", "gft_route_api.cpp", "route_host.cpp", "gft_spans_api.cpp", "spans_host.cpp", "gft_lowermap_api.cpp", "lowermap_host.cpp", "gft_span_runs.cpp", "gft_doc_gather.cpp", "gft_excerpt_api.cpp", "excerpt_host.cpp", "gft_mark_api.cpp", "mark_host.cpp", "gft_replace_api.cpp", "replace_host.cpp", "gft_term_list.cpp", "gft_stats_api.cpp", "stats_host.cpp", "gft_rank_api.cpp", "rank_host.cpp", "gft_words_api.cpp", "words_host.cpp", "witness_terms.cpp", "gft_debug.cpp",
               "gft_multi.cpp", "ac_tables.cpp", "scan2_tables.cpp", "scan3_tables.cpp", "dsl_compile.cpp", "finder_host.cpp", "json_mini.cpp", "group_dsl.cpp", "group_host.cpp", "group_records.cpp", "group_json.cpp", "group_tags.cpp", "group_api.cpp", "host_solve.cpp", "compact_host.cpp", "program_set.cpp", "table_set.cpp", "batch_verdict.cpp", "solve_plan.cpp", "tolower_host.cpp", "rule_set.cpp", "tag_entries.cpp", "rules_json.cpp", "tags_json.cpp", "json_schema.cpp", "json_paths.cpp"]


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_lib(force=False, verbose=False):
    srcs = [os.path.join(CSRC, f) for f in HIP_SOURCES + CXX_SOURCES if os.path.exists(os.path.join(CSRC, f))]
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".h"))]
    hdrs.append(os.path.join(os.path.dirname(HERE), "include", "gft.h"))
    flags = "extra=%d" % int(EXTRA)
    if not os.path.exists(STAMP) or open(STAMP).read() != flags:
        force = True                 # (another set of kernels than the objects on disk were built for)
    if not force and not _newer(LIB, srcs + hdrs):
        return LIB
    objs, jobs = [], []
    for s in srcs:
        o = os.path.join(CSRC, os.path.basename(s) + ".o")
        if force or _newer(o, [s] + hdrs):
            cmd = ["hipcc", "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-Wall", "-c", s, "-o", o]
            if EXTRA:
                cmd.insert(1, "-DGFT_EXTRA_KERNELS")
            if s.endswith(".cpp"):
                cmd[1:1] = ["-x", "hip"]   # host code that includes hip_runtime.h; no kernels inside
            jobs.append(cmd)
        objs.append(o)
    if jobs:
        # (a handful of translation units, the kernels take a minute each: compile them side by side)
        from concurrent.futures import ThreadPoolExecutor

        def run(cmd):
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
        with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as ex:
            list(ex.map(run, jobs))
    cmd = ["hipcc", "-shared", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    with open(STAMP, "w") as f:
        f.write(flags)
    return LIB


def build_all(force=False, verbose=False):
    lib = build_lib(force, verbose)
    from . import workload
    wl = workload.build(force)
    return lib, wl


if __name__ == "__main__":
    print(build_all(force="--force" in sys.argv, verbose=True))
