"""Every launch, asynchronous copy, memset and event of the library goes to the context's stream (include/elfihip.h: the
`_dev` entry points "enqueue on the context's stream and return without synchronising"), and nothing blocks the device
behind the caller's back.  A source check: tests/test_stream_order_gpu.py shows the same property on a busy stream for the
paths its cases take, this one holds every call site, taken or not.

A stream argument is the context's when it is
  * `<something>->stream` (ctx->stream, gp->ctx->stream, h->ctx->stream, ...),
  * a local or a parameter of type hipStream_t: a local must be initialised, in the same file, from an expression that is
    itself the context's; a parameter is checked at its call sites by the C++ type and by this rule applied there,
  * `hi_stream` / `bulk_stream` of the context, inside gp_fit.hip only (its fork-join is joined back with events).
The null stream (0, nullptr, NULL, hipStreamDefault, hipStreamPerThread) is never the context's.

Limits of the rule, enough for the sources as they are: names are resolved per FILE, not per function -- an identifier that
is a hipStream_t parameter anywhere in a file counts as the context's stream everywhere in it (its call sites are checked
instead: test_stream_parameters_receive_the_contexts_stream), the initialisers of a name are collected over the whole file,
and any `x->stream` counts.  So a local declared WITHOUT an initialiser (`hipStream_t s;`, assigned later) that shares its
name with a parameter of the same file would pass; test_no_stream_is_declared_without_an_initialiser keeps that form out.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'elfi_amd', 'csrc')

# call -> position of its stream argument
STREAM_ARG = {'hipLaunchKernelGGL': 4, 'hipMemcpyAsync': 4, 'hipMemcpy2DAsync': 7, 'hipMemsetAsync': 3, 'hipEventRecord': 1,
              'hipStreamWaitEvent': 0, 'hipMemcpyDtoDAsync': 3, 'hipMemcpyHtoDAsync': 3, 'hipMemcpyDtoHAsync': 3,
              'hipMemsetD32Async': 3, 'hipMemsetD8Async': 3, 'hipLaunchCooperativeKernel': 5}
BLOCKING = ('hipMemcpy', 'hipMemcpy2D', 'hipMemset', 'hipDeviceSynchronize', 'hipMemcpyHtoD', 'hipMemcpyDtoH',
            'hipMemcpyDtoD', 'hipMemcpyToSymbol', 'hipMemcpyFromSymbol')
NULL_STREAMS = {'0', 'nullptr', 'NULL', 'hipStreamDefault', 'hipStreamPerThread', 'hipStreamLegacy', '(hipStream_t)0',
                'hipStream_t{}', 'hipStream_t()'}
FORK_JOIN = {'gp_fit.hip': ('hi_stream', 'bulk_stream')}


def sources():
    files = sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.hpp')))
    assert len(files) > 20, 'elfi_amd/csrc not found'
    return files


def strip_comments(text):
    """Comments and string / character literals replaced by blanks of the same length, newlines kept: offsets and line
    numbers stay those of the file."""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        two = text[i:i + 2]
        if two == '//':
            j = text.find('\n', i)
            j = n if j < 0 else j
            out.append(' ' * (j - i))
            i = j
        elif two == '/*':
            j = text.find('*/', i + 2)
            j = n if j < 0 else j + 2
            out.append(''.join(ch if ch == '\n' else ' ' for ch in text[i:j]))
            i = j
        elif c in '"\'':
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == '\\' else 1
            j = min(j + 1, n)
            # a digit separator (1'000'000) is no literal
            if c == '\'' and i > 0 and text[i - 1].isalnum():
                out.append(c)
                i += 1
                continue
            out.append(c + ' ' * (j - i - 2) + c if j - i >= 2 else c)
            i = j
        else:
            out.append(c)
            i += 1
    return ''.join(out)


def split_args(text, open_paren):
    """Arguments of the call whose '(' is at text[open_paren], split at the commas of depth one -- parentheses, brackets
    and braces nest, angle brackets do not (a template argument list in a launch is wrapped in parentheses, or the
    preprocessor would split it too).  -> (list of stripped arguments, offset behind the closing parenthesis)."""
    assert text[open_paren] == '('
    depth, args, start = 0, [], open_paren + 1
    for i in range(open_paren, len(text)):
        c = text[i]
        if c in '([{':
            depth += 1
        elif c in ')]}':
            depth -= 1
            if depth == 0:
                last = text[start:i].strip()
                if last or args:
                    args.append(last)
                return [' '.join(a.split()) for a in args], i + 1
        elif c == ',' and depth == 1:
            args.append(text[start:i].strip())
            start = i + 1
    raise AssertionError('unbalanced call at offset %d' % open_paren)


def calls(text, names):
    """(name, line number, arguments) of every call of one of `names` in comment-free text."""
    pat = re.compile(r'(?<![\w:.>])(?:::)?(%s)\s*\(' % '|'.join(sorted(names, key=len, reverse=True)))
    for mo in pat.finditer(text):
        args, _ = split_args(text, mo.end() - 1)
        yield mo.group(1), text.count('\n', 0, mo.start()) + 1, args


_FUNC = re.compile(r'^[A-Za-z_][\w:<>,*&\s]*?\b([A-Za-z_]\w*)\s*\([^;{}]*\)\s*(?:const\s*)?(?:noexcept\s*)?\{', re.M)


def enclosing_function(text, line):
    """Name of the last function definition that starts at column 0 at or before `line` (the files' style: every
    definition starts a line, bodies are indented)."""
    name = None
    for mo in _FUNC.finditer(text):
        if text.count('\n', 0, mo.start()) + 1 > line:
            break
        if mo.group(1) not in ('if', 'for', 'while', 'switch'):
            name = mo.group(1)
    return name


def enclosing_scope(text, pos):
    """The text of the line that opens the innermost brace scope around `pos` (to tell a struct member from a local)."""
    depth = 0
    for i in range(pos - 1, -1, -1):
        if text[i] == '}':
            depth += 1
        elif text[i] == '{':
            if depth == 0:
                return text[text.rfind('\n', 0, i) + 1:i]
            depth -= 1
    return ''


def stream_locals(text):
    """name -> list of initialisers, of every hipStream_t variable the file declares with one; hipStream_t parameters
    (declared without initialiser, followed by ',' or ')') -> name -> []."""
    inits, params = {}, set()
    for mo in re.finditer(r'\bhipStream_t\s+(?:const\s+)?([^;(){}]*?=[^;{}]*?);', text):      # hipStream_t a = x, b = y;
        for decl in split_args('(' + mo.group(1) + ')', 0)[0]:
            name, _, init = decl.partition('=')
            if init:
                inits.setdefault(name.strip(), []).append(init.strip())
    for mo in re.finditer(r'\bhipStream_t\s+(?:const\s+)?(\w+)\s*[,)]', text):
        params.add(mo.group(1))
    return inits, params


def is_context_stream(expr, fname, inits, params, seen=()):
    expr = expr.strip()
    while expr.startswith('(') and expr.endswith(')') and split_args(expr, 0)[1] == len(expr):
        expr = expr[1:-1].strip()
    if expr in NULL_STREAMS:
        return False
    if re.fullmatch(r'[\w.\->]*\bctx\s*->\s*stream|ctx\.stream|[\w.\->]+->stream', expr):
        return True
    for member in FORK_JOIN.get(fname, ()):
        if re.fullmatch(r'[\w.\->]*\bctx\s*->\s*%s' % member, expr):
            return True
    if re.fullmatch(r'\w+', expr) and expr not in seen:
        if expr in inits:
            return all(is_context_stream(e, fname, inits, params, seen + (expr,)) for e in inits[expr])
        if expr in params:
            return True
    # a choice between two streams of the context
    mo = re.fullmatch(r'(.+?)\?(.+):(.+)', expr)
    if mo:
        return all(is_context_stream(e, fname, inits, params, seen) for e in mo.groups()[1:])
    return False


def stream_sites():
    """(file, line, call, stream expression, is the context's) of every stream-taking call."""
    out = []
    for path in sources():
        fname = os.path.basename(path)
        text = strip_comments(open(path).read())
        inits, params = stream_locals(text)
        for name, line, args in calls(text, STREAM_ARG):
            pos = STREAM_ARG[name]
            expr = args[pos] if len(args) > pos else ''      # (a missing stream argument defaults to the null stream)
            out.append((fname, line, name, expr, bool(expr) and is_context_stream(expr, fname, inits, params)))
    return out


def test_the_splitter_keeps_template_commas_and_nested_calls():
    text = 'hipLaunchKernelGGL((k<A, B>), dim3(g, 1), dim3(64), f(a, b), ctx->stream, x[i, j], T{1, 2});'
    args, end = split_args(text, text.index('('))
    assert args == ['(k<A, B>)', 'dim3(g, 1)', 'dim3(64)', 'f(a, b)', 'ctx->stream', 'x[i, j]', 'T{1, 2}']
    assert text[end:] == ';'
    assert split_args('f()', 1) == ([], 3)
    text = strip_comments('a /* hipMemcpy( */ "hipMemset(" // hipMemcpy(\nhipMemcpy(d, s, 8, k);')
    assert [(n, ln) for n, ln, _ in calls(text, BLOCKING)] == [('hipMemcpy', 2)]
    assert [n for n, _, _ in calls('hipMemcpyAsync(a); my_hipMemcpy(b); x.hipMemcpy(c); hipMemcpy (d);', BLOCKING)] == ['hipMemcpy']


def test_the_stream_rule_tells_the_streams_apart():
    inits, params = stream_locals('hipStream_t st = ctx->stream; hipStream_t bad = 0; hipStream_t two = st;\n'
                                  'void f(hipStream_t s, int n) {} hipStream_t other = make();')
    assert params == {'s'}
    ok = lambda e, f='x.hip': is_context_stream(e, f, inits, params)
    assert ok('ctx->stream') and ok('gp->ctx->stream') and ok('st') and ok('two') and ok('s') and ok('(st)')
    assert not ok('0') and not ok('nullptr') and not ok('bad') and not ok('other') and not ok('') and not ok('unknown')
    assert not ok('ctx->hi_stream') and ok('ctx->hi_stream', 'gp_fit.hip') and ok('gp->ctx->bulk_stream', 'gp_fit.hip')
    assert ok('big ? ctx->stream : st') and not ok('big ? ctx->stream : 0')


def uninitialised_stream_locals(text):
    """(line, declaration) of every `hipStream_t s;` / `hipStream_t a, b;` that is not a member of a struct or class."""
    out = []
    for mo in re.finditer(r'\bhipStream_t\s+(?:const\s+)?\w+(?:\s*,\s*\w+)*\s*;', text):
        if not re.search(r'\b(struct|class)\b', enclosing_scope(text, mo.start())):
            out.append((text.count('\n', 0, mo.start()) + 1, mo.group(0)))
    return out


def test_no_stream_is_declared_without_an_initialiser():
    """`hipStream_t s;` (assigned later, from anything) is the one form the per-file rule cannot follow."""
    sample = 'struct P {\n  hipStream_t own;\n};\nint f(hipStream_t st) {\n  hipStream_t s;\n  hipStream_t t = st;\n  s = 0;\n}\n'
    assert uninitialised_stream_locals(sample) == [(5, 'hipStream_t s;')]
    bad = ['%s:%d %s' % ((os.path.basename(path),) + hit) for path in sources()
           for hit in uninitialised_stream_locals(strip_comments(open(path).read()))]
    assert not bad, 'a stream variable without an initialiser:\n' + '\n'.join(bad)


def test_every_stream_argument_is_the_contexts():
    sites = stream_sites()
    assert len(sites) > 200, 'the scan found too few call sites to be looking at the library'
    assert {s[2] for s in sites} >= {'hipLaunchKernelGGL', 'hipMemcpyAsync', 'hipMemsetAsync', 'hipEventRecord', 'hipStreamWaitEvent'}
    bad = ['%s:%d %s on `%s`' % s[:4] for s in sites if not s[4]]
    assert not bad, 'not on the context\'s stream:\n' + '\n'.join(bad)


def test_stream_parameters_receive_the_contexts_stream():
    """A helper that takes `hipStream_t s` is as good as its callers: every call, in any file, of a function with such a
    parameter passes the context's stream in that position."""
    texts = {os.path.basename(p): strip_comments(open(p).read()) for p in sources()}
    helpers = {}      # function name -> positions of its hipStream_t parameters
    for fname, text in texts.items():
        for mo in re.finditer(r'\b([A-Za-z_]\w*)\s*\(', text):
            if mo.group(1) in STREAM_ARG or mo.group(1) in ('if', 'for', 'while', 'switch', 'return', 'sizeof'):
                continue
            try:
                args, end = split_args(text, mo.end() - 1)
            except AssertionError:
                continue
            pos = [i for i, a in enumerate(args) if re.match(r'(const\s+)?hipStream_t\s+\w+$', a)]
            if pos and not all(re.match(r'(const\s+)?[\w:]+[\w\s*&:<>]*\s+[*&]*\w+(\s*=.*)?$', a) for a in args):
                continue      # (not a parameter list)
            if pos:
                helpers.setdefault(mo.group(1), set()).update(pos)
    assert 'sweep_plan' in helpers, 'the scan no longer finds the helpers that take a stream'
    bad = []
    for fname, text in texts.items():
        inits, params = stream_locals(text)
        for name, line, args in calls(text, helpers) if helpers else ():
            if any(re.match(r'(const\s+)?hipStream_t\s+\w+$', a) for a in args):
                continue      # the definition or a declaration
            for pos in helpers[name]:
                if pos < len(args) and not is_context_stream(args[pos], fname, inits, params):
                    bad.append('%s:%d %s(... `%s` ...)' % (fname, line, name, args[pos]))
    assert not bad, 'a helper is handed a stream that is not the context\'s:\n' + '\n'.join(bad)


# file -> {enclosing function: (calls, why the device may be blocked there)}
ALLOWED_BLOCKING = {
    'gp_hyper.hip': {
        'hyper_grad_impl': (['hipMemcpy'], 'the work list of a padded size, uploaded once per size from a local vector; the '
                                           'stream is synchronised first because a launch in flight may read the old list'),
    },
    'gp_fit.hip': {
        'sweep_plan': (['hipMemcpy'] * 3, 'the sweep schedule of a (blocks, workgroups) pair, uploaded when the pair changes; '
                                          'the stream is synchronised first because a sweep in flight may read the old table'),
    },
}


def blocking_sites():
    out = []
    for path in sources():
        fname = os.path.basename(path)
        text = strip_comments(open(path).read())
        for name, line, args in calls(text, BLOCKING):
            out.append((fname, enclosing_function(text, line), name, line))
    return out


def test_blocking_calls_are_the_listed_ones():
    found = {}
    for fname, func, name, line in blocking_sites():
        found.setdefault((fname, func), []).append(name)
    listed = {(f, fn): sorted(calls_) for f, funcs in ALLOWED_BLOCKING.items() for fn, (calls_, why) in funcs.items()}
    extra = {k: v for k, v in found.items() if sorted(v) != listed.get(k)}
    assert not extra, 'blocking device calls outside the allow-list (use the Async form on the context\'s stream): %r' % extra
    gone = sorted(set(listed) - set(found))
    assert not gone, 'the allow-list names sites that no longer block; shorten it: %r' % gone


def test_allowed_blocking_calls_follow_a_synchronisation_of_the_contexts_stream():
    """What makes the listed sites harmless: the function has waited for the context's stream before it blocks, so the
    null-stream copy cannot overtake (or be overtaken by) work of the context."""
    for path in sources():
        fname = os.path.basename(path)
        if fname not in ALLOWED_BLOCKING:
            continue
        text = strip_comments(open(path).read())
        lines = text.split('\n')
        for _, func, name, line in [s for s in blocking_sites() if s[0] == fname]:
            start = max(i for i, mo in ((text.count('\n', 0, mo.start()) + 1, mo) for mo in _FUNC.finditer(text))
                        if i <= line and mo.group(1) == func)
            body = '\n'.join(lines[start - 1:line - 1])
            inits, params = stream_locals(text)
            waited = [a[0] for n_, _, a in calls(body, ('hipStreamSynchronize',)) if a]
            assert any(is_context_stream(e, fname, inits, params) for e in waited), \
                '%s:%d %s in %s is not behind a synchronisation of the context\'s stream' % (fname, line, name, func)
