"""include/airwave_hip.h, "stream order": every device entry only enqueues on the context's stream.  Source-level part (CPU), the
companion of tests/test_gpu_stream_order.py: every kernel launch in csrc/device passes a stream that its launcher was handed, every
asynchronous HIP call of the two runtime units names the context's stream (or one of the host pipeline's, which are ordered against it by
events), and blocking copies and memsets occur only where the list below says, so that a new one on a process path fails with the
function's name."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airwave_amd", "csrc")

KEYWORDS = {"if", "for", "while", "switch", "catch", "return", "sizeof", "else", "do", "constexpr"}


def blank_comments_and_strings(src: str) -> str:
    """The source with comments, string and character literals replaced by spaces: offsets and line numbers stay."""
    out, i, n = list(src), 0, len(src)
    while i < n:
        two = src[i:i + 2]
        if two == "//":
            j = src.find("\n", i)
            j = n if j < 0 else j
        elif two == "/*":
            j = src.find("*/", i + 2)
            j = n if j < 0 else j + 2
        elif src[i] in "\"'":
            j = i + 1
            while j < n and src[j] != src[i]:
                j += 2 if src[j] == "\\" else 1
            j += 1
        else:
            i += 1
            continue
        for k in range(i, min(j, n)):
            if out[k] != "\n":
                out[k] = " "
        i = j
    return "".join(out)


def header_name(header: str):
    """The name of the function whose body follows `header`: the identifier in front of the header's last parenthesised group (behind
    which only words such as const, noexcept, override or try may stand).  None for control statements, lambdas and brace initialisers."""
    close = header.rfind(")")
    if close < 0 or not re.fullmatch(r"[\s\w]*", header[close + 1:]):
        return None
    depth = 0
    for i in range(close, -1, -1):
        depth += {")": 1, "(": -1}.get(header[i], 0)
        if depth == 0:
            m = re.search(r"([A-Za-z_]\w*)\s*$", header[:i])
            return m.group(1) if m and m.group(1) not in KEYWORDS else None
    return None


def functions(code: str):
    """Every function definition of `code` (comments blanked) as (name, header, start, end): header is the text in front of the body's
    brace (the parameter list is in it), start / end the offsets of the body's braces.  Members of classes and lambdas-free nesting are
    found too; control statements, lambdas and brace initialisers are no functions."""
    found, stack, last = [], [], 0           # last: offset behind the last ; { or }
    for i, ch in enumerate(code):
        if ch == ";":
            last = i + 1
        elif ch == "{":
            header = code[last:i]
            stack.append((header_name(header), header, i))
            last = i + 1
        elif ch == "}":
            name, header, start = stack.pop()
            if name:
                found.append((name, header, start, i))
            last = i + 1
    assert not stack
    return found


def enclosing(funcs, pos):
    """The innermost function whose body holds offset pos."""
    best = None
    for f in funcs:
        if f[2] < pos < f[3] and (best is None or f[2] > best[2]):
            best = f
    return best


def call_args(code: str, open_paren: int, close: str = ")"):
    """The top-level arguments of the call whose '(' (or the first '<' of '<<<') stands at open_paren, and the offset behind it."""
    args, depth, cur, i = [], 0, [], open_paren + 1
    while True:
        ch = code[i]
        if depth == 0 and (ch == close and (close == ")" or code[i:i + 3] == ">>>")):
            args.append("".join(cur).strip())
            return args, i + 1
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            args.append("".join(cur).strip())
            cur = []
        else:
            cur.append(ch)
        i += 1


def line_of(code, pos):
    return code.count("\n", 0, pos) + 1


def sources(sub, suffixes):
    d = os.path.join(CSRC, sub) if sub else CSRC
    return sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith(suffixes))


# ---- 1. kernel launches --------------------------------------------------------------------------------------------------------------

# a launch form -> the index of its stream argument: the chevron form, the HIP macro, and the kernel tables' launch() (launch_table.hpp)
LAUNCH_FORMS = [(re.compile(r"<<<"), 3, ">"), (re.compile(r"\bhipLaunchKernelGGL\s*\("), 4, ")"), (re.compile(r"(?<![\w.>])launch\s*\("), 3, ")"),
                (re.compile(r"\bk\.launch\s*\("), 4, ")")]          # (and the long-window split rows' launch pointer, lw_kernels.hip)


def launch_sites(code):
    for rx, index, close in LAUNCH_FORMS:
        for m in rx.finditer(code):
            if close == ")" and re.search(r"\bvoid\s+$", code[max(0, m.start() - 16):m.start()]):
                continue                     # (launch_table.hpp's definition of launch(), whose own launch is a site of its own)
            args, _ = call_args(code, m.end() - 1 if close == ")" else m.end() - 1, close)
            yield m.start(), index, args


def check_device_file(path):
    """-> (launch sites, problems) of one device source."""
    code = blank_comments_and_strings(open(path).read())
    funcs = functions(code)
    rel = os.path.relpath(path, CSRC)
    sites, bad = 0, []
    for pos, index, args in launch_sites(code):
        sites += 1
        where = f"{rel}:{line_of(code, pos)}"
        if len(args) <= index:
            bad.append(f"{where}: a launch without a stream argument")
            continue
        stream = args[index]
        if not re.fullmatch(r"[A-Za-z_]\w*", stream) or stream in ("nullptr", "NULL", "hipStreamDefault", "hipStreamLegacy", "hipStreamPerThread"):
            bad.append(f"{where}: launches on {stream!r}, which is no stream parameter")
            continue
        f = enclosing(funcs, pos)
        if f is None or not re.search(r"\bhipStream_t\s+" + stream + r"\s*[,)]", f[1] + ")"):
            bad.append(f"{where}: {stream!r} is not a hipStream_t parameter of {f[0] if f else 'any function'}")
    # a stream is only ever handed down: no device source makes, names or defaults one
    for m in re.finditer(r"\bhipStream_t\b(?!\s*(?:[A-Za-z_]\w*\s*)?[,)])|\bhipStream(?:Create\w*|Default|Legacy|PerThread)\b", code):
        bad.append(f"{rel}:{line_of(code, m.start())}: {code[m.start():m.start() + 40].split(chr(10))[0]!r}: a stream that is no parameter")
    return sites, bad


def test_every_kernel_launch_runs_on_the_stream_its_launcher_was_handed():
    total, bad = 0, []
    for path in sources("device", (".hip", ".hpp")):
        n, b = check_device_file(path)
        total += n
        bad += b
    assert not bad, "\n".join(bad)
    assert total >= 40, total               # (the scan found the launches: 44 sites when this was written)


# ---- 2. asynchronous HIP calls of the runtime units ------------------------------------------------------------------------------------

# call -> the index of its stream argument (-1: the last)
ASYNC_CALLS = {"hipMemcpyAsync": -1, "hipMemsetAsync": -1, "hipMemsetD32Async": -1, "hipMemcpy2DAsync": -1, "hipEventRecord": 1,
               "hipStreamWaitEvent": 0, "hipStreamSynchronize": 0}
CONTEXT_STREAM = re.compile(r"(?:\w+(?:->|\.))*(?:c|ctx)->stream")               # c->stream, ctx->stream, sp->ctx->stream, s.ctx->stream, eq->ctx->stream
PIPELINE_STREAM = re.compile(r"(?:c|ctx)->s_(?:h2d|d2h)|s2")                      # the host entry's copy streams; the PCIe probe's second stream


def stream_ok(expr, body, pipeline=True):
    """pipeline: the copy streams count (copies and events); kernels run on the context's stream alone."""
    expr = expr.strip()
    if "?" in expr:                          # a choice between two streams: both
        a, b = expr.split("?", 1)[1].split(":", 1)
        return stream_ok(a, body, pipeline) and stream_ok(b, body, pipeline)
    if CONTEXT_STREAM.fullmatch(expr) or (pipeline and PIPELINE_STREAM.fullmatch(expr)):
        return True
    # a local alias: `hipStream_t s = <the context's stream>;` in the same function, and never assigned again
    m = re.search(r"\bhipStream_t\s+(?:const\s+)?" + re.escape(expr) + r"\s*=\s*([^;]+);", body) if re.fullmatch(r"[A-Za-z_]\w*", expr) else None
    return bool(m and CONTEXT_STREAM.fullmatch(m.group(1).strip()) and not re.search(r"(?<![\w>.])" + re.escape(expr) + r"\s*=[^=]", body[m.end():]))


def check_runtime_file(path):
    code = blank_comments_and_strings(open(path).read())
    funcs = functions(code)
    rel = os.path.relpath(path, CSRC)
    sites, bad = 0, []
    for m in re.finditer(r"\b(" + "|".join(ASYNC_CALLS) + r"|awk::launch_\w+)\s*\(", code):
        f = enclosing(funcs, m.start())
        assert f, (rel, line_of(code, m.start()))
        args, _ = call_args(code, m.end() - 1)
        body = code[f[2]:f[3]]
        where = f"{rel}:{line_of(code, m.start())} ({f[0]})"
        sites += 1
        if m.group(1).startswith("awk::"):      # a launcher of csrc/device: one of its arguments is the stream
            if not any(stream_ok(a, body, pipeline=False) for a in args if "stream" in a or re.fullmatch(r"s\d?", a)):
                bad.append(f"{where}: {m.group(1)} is handed no stream of the context")
        elif not stream_ok(args[ASYNC_CALLS[m.group(1)]], body):
            bad.append(f"{where}: {m.group(1)} on {args[ASYNC_CALLS[m.group(1)]]!r}")
    return sites, bad


def test_every_asynchronous_call_of_the_runtime_names_the_contexts_stream():
    total, bad = 0, []
    for rel in ("runtime.cpp", "eq_runtime.cpp"):
        n, b = check_runtime_file(os.path.join(CSRC, rel))
        total += n
        bad += b
    assert not bad, "\n".join(bad)
    assert total >= 100, total               # (the scan found the calls: 112 when this was written)


# ---- 3. blocking copies and memsets ------------------------------------------------------------------------------------------------------

# (file, function) -> blocking hipMemcpy* / hipMemset* calls it may hold.  Uploads made while something is created (Buf::upload: tables and
# twiddles; prepare_state: an equalizer's tables) and read-backs behind a hipStreamSynchronize of the context's stream (the record
# getters through get_field, the loudness getters, the debug stamps, and the single-stream page-locked path, which has synchronised by then).
BLOCKING_ALLOWED = {
    ("host/device_buf.hpp", "upload"): 1,
    ("eq_runtime.cpp", "prepare_state"): 1,
    ("runtime.cpp", "get_field"): 1,
    ("runtime.cpp", "aw_spatializer_get_loudness"): 1,
    ("runtime.cpp", "aw_spatializer_get_loudness_hops"): 1,
    ("runtime.cpp", "aw_spatializer_debug_stamps"): 1,
    ("runtime.cpp", "batch_run_pinned"): 1,
    ("runtime.cpp", "lim_host_call"): 1,
}
# ... of which these synchronise the context's stream in their own body, in front of the copy
SYNCHRONISE_FIRST = ("aw_spatializer_get_loudness_hops", "aw_spatializer_debug_stamps", "batch_run_pinned")
BLOCKING = re.compile(r"\b(hipMem(?:cpy|set)(?!\w*Async)\w*)\s*\(")


def blocking_calls(csrc=None):
    """{(file, function): count} over every source of the library."""
    csrc, seen = csrc or CSRC, {}
    for sub in ("", "host", "device"):
        d = os.path.join(csrc, sub)
        for name in sorted(os.listdir(d)):
            if not name.endswith((".cpp", ".hpp", ".hip", ".h")):
                continue
            code = blank_comments_and_strings(open(os.path.join(d, name)).read())
            funcs = functions(code)
            for m in BLOCKING.finditer(code):
                f = enclosing(funcs, m.start())
                key = (os.path.join(sub, name) if sub else name, f[0] if f else "<file scope>")
                seen[key] = seen.get(key, 0) + 1
    return seen


def test_blocking_copies_only_where_the_list_says():
    seen = blocking_calls()
    for key, n in sorted(seen.items()):
        assert key in BLOCKING_ALLOWED, f"{key[1]} ({key[0]}) makes a blocking hipMemcpy / hipMemset: process paths copy with the Async forms on the context's stream"
        assert n == BLOCKING_ALLOWED[key], f"{key[1]} ({key[0]}) makes {n} blocking copies, the list allows {BLOCKING_ALLOWED[key]}"
    assert sorted(seen) == sorted(BLOCKING_ALLOWED), sorted(set(BLOCKING_ALLOWED) - set(seen))          # (the list holds nothing stale)
    code = blank_comments_and_strings(open(os.path.join(CSRC, "runtime.cpp")).read())
    by_name = {f[0]: code[f[2]:f[3]] for f in functions(code)}
    for fn in SYNCHRONISE_FIRST:
        body = by_name[fn]
        sync, copy = body.find("hipStreamSynchronize(sp->ctx->stream)"), BLOCKING.search(body).start()
        assert 0 <= sync < copy, fn
    # the record getters read through get_field behind get_begin, which synchronises the context's stream under the launch lock
    assert "hipStreamSynchronize(sp->ctx->stream)" in by_name["get_begin"]
    for fn, body in by_name.items():
        if "get_field(" in body and fn != "get_field":
            assert 0 <= body.find("get_begin(") < body.find("get_field("), fn


def test_the_zero_page_is_written_on_the_contexts_stream():
    """d_zeros is what the tile kernels read as "frames past the end of a call": its one write is ordered on the stream they run on."""
    assert ("runtime.cpp", "context_create_impl") not in BLOCKING_ALLOWED and ("runtime.cpp", "context_create_impl") not in blocking_calls()
    code = blank_comments_and_strings(open(os.path.join(CSRC, "runtime.cpp")).read())
    body = {f[0]: code[f[2]:f[3]] for f in functions(code)}["context_create_impl"]
    assert "hipMemsetAsync(c->d_zeros.get(), 0, 4096, c->stream)" in body


def test_the_scanner_sees_what_it_should():
    """The checks above on small texts of each kind they must refuse."""
    code = blank_comments_and_strings("""
hipError_t launch_a(const P &p, hipStream_t stream) {   // hipLaunchKernelGGL(k, g, b, 0, 0) in a comment
    hipLaunchKernelGGL((k<A, 1>), dim3(a, (unsigned)b), dim3(64), 0, stream, p, "x, y");
    return hipGetLastError();
}
hipError_t launch_b(const P &p, hipStream_t stream) {
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, p);
    k2<<<grid, block, 0>>>(p);
    k3<<<grid, block, 0, other>>>(p);
    return hipGetLastError();
}
struct T { void run(hipStream_t s) { if (x) { launch(*k, grid, dim3(64), s, p); } } };
aw_status getter(aw_spatializer *sp) try {
    aw_status st = get_begin(sp, [](const aw_spatializer *s) { return s->d.get(); }, &lk);
    for (int i = 0; i < 2; ++i) { auto up = [&](auto &buf) { return hipMemcpy(buf, 0); }; }
    return st;
} AW_NOEXCEPT_TAIL
""")
    funcs = functions(code)
    assert [f[0] for f in funcs] == ["launch_a", "launch_b", "run", "getter"]
    assert enclosing(funcs, code.index("hipMemcpy(buf"))[0] == "getter"
    sites = sorted((line_of(code, pos), args[index] if len(args) > index else None) for pos, index, args in launch_sites(code))
    assert sites == [(3, "stream"), (7, "0"), (8, None), (9, "other"), (12, "s")], sites
    body = "{ hipStream_t s = sp->ctx->stream; hipStream_t t = nullptr; hipStream_t u = c->stream; u = other; }"
    assert stream_ok("s", body) and stream_ok("sp->ctx->stream", body) and stream_ok("what == 2 ? s2 : c->stream", body) and stream_ok("c->s_h2d", body)
    assert not stream_ok("t", body) and not stream_ok("u", body) and not stream_ok("0", body) and not stream_ok("nullptr", body) and not stream_ok("sp->stream2", body)
    assert [m.group(1) for m in BLOCKING.finditer("hipMemcpy(a); hipMemcpyAsync(b); hipMemset(c); hipMemcpy2D(d); hipMemsetD32Async(e); hipMemcpyDtoH(f);")] == \
        ["hipMemcpy", "hipMemset", "hipMemcpy2D", "hipMemcpyDtoH"]
