"""What can be held of the stream contract of include/xparcel.h without a GPU.

Census: every entry point the header declares with a trailing `void *stream` is reached by a recipe of tests/stream_cases.py
(the device tests, tests/test_gpu_streams.py, run every recipe on a side stream and check that the declared entry points were
really called), or stands in stream_cases.EXEMPT with a reason.

Source rule: in xarray_parcel_amd/csrc every launch, asynchronous copy, memset, allocation and release names a stream
expression that is not the default stream written out, and the calls that block the host or the device live only in the
functions listed below."""
import os
import re

from tests import stream_cases as S
from xarray_parcel_amd import _lib as L

# the asynchronous calls (launch_columns: csrc/xp_launch.hpp, the launch of all but five kernels) and the (zero-based)
# position of their stream argument
STREAM_ARG = {'launch_columns': 2, 'hipLaunchKernelGGL': 4, 'hipMemcpyAsync': 4, 'hipMemsetAsync': 3, 'hipMallocAsync': 2, 'hipFreeAsync': 1}
DEFAULT_STREAM = re.compile(r'^(\(\s*hipStream_t\s*\)\s*)?\(?\s*(0|NULL|nullptr|hipStreamLegacy|hipStreamPerThread)\s*\)?$')
# the calls that wait for the device, and the only functions that may hold them
BLOCKING = ('hipMemcpy', 'hipMemset', 'hipMalloc', 'hipFree', 'hipDeviceSynchronize')
BLOCKING_ALLOWED = {'xp_init', 'xp_set_tables', 'xp_set_family_table'}       # they replace tables: documented to drain the device
STREAM_SYNC_ALLOWED = {'Stager::finish',          # host buffers: "synchronise the stream before returning"
                       'xp_rebase_profile'}       # "Synchronises the stream": the number of rows comes back to the host
KEYWORDS = {'if', 'for', 'while', 'switch', 'catch', 'return', 'sizeof', 'else', 'do'}


def test_every_stream_entry_point_has_a_recipe():
    declared = S.header_stream_entries()
    assert len(declared) >= 49 and {'xp_cape_cin', 'xp_interp1d', 'xp_ecape', 'xp_storm_proxies'} <= declared, sorted(declared)
    assert not {'xp_init', 'xp_set_tables', 'xp_family_table', 'xp_version', 'xp_last_error'} & declared
    assert declared <= set(L.SYMBOLS)
    reached = set().union(*[r.entries for r in S.RECIPES.values()])
    assert all(isinstance(why, str) and len(why) > 20 for why in S.EXEMPT.values())
    assert set(S.EXEMPT) <= declared and not set(S.EXEMPT) & reached
    missing, unknown = declared - reached - set(S.EXEMPT), reached - declared
    assert not missing, 'entry points that take a stream and have no recipe in tests/stream_cases.py: %s' % sorted(missing)
    assert not unknown, 'recipes declare entry points the header does not have: %s' % sorted(unknown)


def test_recipe_table_is_consistent():
    for name, r in S.RECIPES.items():
        assert r.name == name and r.entries and r.dtypes and callable(r.fn)
    for group in (S.HOST_SUBSET, S.THREAD_RECIPES, S.PERSISTENT, S.OTHER_DEVICE_RECIPES, tuple(S.SYNCHRONISES)):
        assert set(group) <= set(S.RECIPES), set(group) - set(S.RECIPES)
    assert all(S.RECIPES[n].host for n in S.HOST_SUBSET)
    # the persistent recipes sit just over persist()'s thresholds in csrc/xparcel.hip, the shared grid far below them
    with open(os.path.join(L.SRC_DIR, 'xparcel.hip')) as f:
        assert 'searching ? (1ll << 19) : (3ll << 18)' in f.read()
    assert S.RECIPES['persistent_surface'].grid[1] == 3 * 2 ** 18 + 77 and S.RECIPES['persistent_fused'].grid[1] == 2 ** 19 + 77
    assert S.NCOL == 1337 and S.NCOL % 64 and -(-S.NCOL // 256) == 6
    g = S.grid()
    assert g['p'].shape == (S.NLEV, S.NCOL) and (g['z'][1:] > g['z'][:-1]).all() and (g['z'][-1] - g['z'][0] > 6000.0).all()
    assert 0 < int(S.np.isnan(g['t']).any(0).sum()) < S.NCOL // 4 and 0 < int(S.np.isnan(g['u']).sum())


# ---- the source rule -------------------------------------------------------------------------------------------------------
def _blank(m):
    return re.sub(r'[^\n]', ' ', m.group(0))


def strip_comments_and_strings(text):
    """The same text with comments and string literals blanked, every character and line where it was."""
    return re.sub(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\\n])*"', _blank, text, flags=re.S)


def call_arguments(text, start):
    """The top-level arguments of the call whose opening parenthesis is at text[start]."""
    depth, args, last = 0, [], start + 1
    for i in range(start, len(text)):
        ch = text[i]
        if ch in '([{':
            depth += 1
        elif ch in ')]}':
            depth -= 1
            if depth == 0:
                args.append(text[last:i].strip())
                return args
        elif ch == ',' and depth == 1:
            args.append(text[last:i].strip())
            last = i + 1
    raise AssertionError('unbalanced call')


def join_template_arguments(args):
    """call_arguments' pieces with the commas of a kernel's template arguments put back: launch_columns(k<T, N>, n, s, ...)."""
    out = []
    for a in args:
        if out and out[-1].count('<') > out[-1].count('>'):
            out[-1] += ', ' + a
        else:
            out.append(a)
    return out


HEADER = re.compile(r'(~?\w[\w]*)\s*\([^;{}]*\)\s*(?:const\s*)?(?:noexcept\s*)?(?::[^;{}]*)?$', re.S)
RECORD = re.compile(r'\b(?:struct|class)\s+(\w+)[^;{}()]*$', re.S)


def enclosing_functions(text):
    """For every character of the (comment-free) text the function it lies in: 'name' or 'Record::name' -- the outermost
    function body around it, so a lambda or a block inside a function belongs to that function -- or None."""
    owner, stack, seg = [None] * len(text), [], 0
    for i, ch in enumerate(text):
        if ch == '{':
            head = text[seg:i]
            f, r = HEADER.search(head), RECORD.search(head)
            if f and f.group(1) not in KEYWORDS:
                stack.append(('fn', f.group(1)))
            elif r:
                stack.append(('record', r.group(1)))
            else:
                stack.append(('block', None))
            seg = i + 1
        elif ch == '}':
            if stack:
                stack.pop()
            seg = i + 1
        elif ch == ';':
            seg = i + 1
        fn = next((j for j, (kind, _) in enumerate(stack) if kind == 'fn'), None)
        if fn is not None:
            rec = next((name for kind, name in reversed(stack[:fn]) if kind == 'record'), None)
            owner[i] = (rec + '::' if rec else '') + stack[fn][1]
    return owner


def scan_sources(sources):
    """Every violation of the source rule in {path: text} as 'path:line: what'."""
    bad = []
    for path, raw in sorted(sources.items()):
        text = strip_comments_and_strings(raw)
        owner = enclosing_functions(text)
        where = lambda pos: '%s:%d' % (path, text.count('\n', 0, pos) + 1)
        for m in re.finditer(r'\b(hip\w+|launch_columns)\s*\(', text):
            name, pos = m.group(1), m.start()
            if name in STREAM_ARG:
                args = call_arguments(text, m.end() - 1)
                if name == 'launch_columns':
                    args = join_template_arguments(args)
                if len(args) <= STREAM_ARG[name]:
                    bad.append('%s: %s names no stream (%d arguments)' % (where(pos), name, len(args)))
                elif DEFAULT_STREAM.match(args[STREAM_ARG[name]]):
                    bad.append('%s: %s on the default stream (%r)' % (where(pos), name, args[STREAM_ARG[name]]))
            elif name in BLOCKING and owner[pos] not in BLOCKING_ALLOWED:
                bad.append('%s: blocking %s in %s' % (where(pos), name, owner[pos]))
            elif name == 'hipStreamSynchronize' and owner[pos] not in STREAM_SYNC_ALLOWED:
                bad.append('%s: hipStreamSynchronize in %s' % (where(pos), owner[pos]))
    return bad


def csrc_sources():
    out = {}
    for f in sorted(os.listdir(L.SRC_DIR)):
        if f.endswith(('.hip', '.hpp')):
            with open(os.path.join(L.SRC_DIR, f)) as fh:
                out['xarray_parcel_amd/csrc/' + f] = fh.read()
    return out


def test_source_rule():
    sources = csrc_sources()
    text = '\n'.join(strip_comments_and_strings(s) for s in sources.values())
    # the scan sees what it is meant to see: the launch sites and the allowed waits are all there
    assert len(re.findall(r'\bhipLaunchKernelGGL\s*\(', text)) >= 5 and len(re.findall(r"\blaunch_columns\s*\(", text)) >= 44
    assert len(re.findall(r'\bhipStreamSynchronize\s*\(', text)) == 3 and len(re.findall(r'\bhipDeviceSynchronize\s*\(', text)) == 3
    bad = scan_sources(sources)
    assert not bad, '\n' + '\n'.join(bad)


def test_source_rule_sees_violations():
    """The scan on doctored copies of the sources (in memory): each kind of violation is reported with file and line."""
    sources = csrc_sources()
    path = 'xarray_parcel_amd/csrc/xparcel.hip'
    src = sources[path]

    def doctored(old, new):
        assert src.count(old) == 1, old
        return scan_sources({path: src.replace(old, new)})          # (the other files: test_source_rule)
    line = lambda old: src[:src.index(old)].count('\n') + 1
    old = 'launch_columns(xp::k_per_point<decltype(z), Op>, n, st.s, a)'
    for zero in ('0', 'nullptr', '(hipStream_t)0', 'NULL'):
        bad = doctored(old, old.replace('st.s', zero))
        assert bad == ['%s:%d: launch_columns on the default stream (%r)' % (path, line(old), zero)], bad
    assert doctored(old, old.replace(', st.s, a', '')) == ['%s:%d: launch_columns names no stream (2 arguments)' % (path, line(old))]
    old = 'hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, s)'
    assert doctored(old, 'hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice)') == \
        ['%s:%d: hipMemcpyAsync names no stream (4 arguments)' % (path, line(old))]
    assert doctored(old, 'hipMemcpy(d, p, bytes, hipMemcpyHostToDevice)') == ['%s:%d: blocking hipMemcpy in Stager::in' % (path, line(old))]
    old = 'HIP_TRY(hipMallocAsync(&v, bytes ? bytes : 1, s));'
    assert doctored(old, old + ' HIP_TRY(hipDeviceSynchronize());') == ['%s:%d: blocking hipDeviceSynchronize in Stager::alloc' % (path, line(old))]
    assert doctored(old, 'HIP_TRY(hipMalloc(&v, bytes ? bytes : 1));') == ['%s:%d: blocking hipMalloc in Stager::alloc' % (path, line(old))]
    assert doctored(old, old.replace(', s)', ', 0)')) == ["%s:%d: hipMallocAsync on the default stream ('0')" % (path, line(old))]
    old = '~Stager() { for (void *p : scratch) (void)hipFreeAsync(p, s); }'
    assert doctored(old, old.replace('hipFreeAsync(p, s)', 'hipFree(p)')) == ['%s:%d: blocking hipFree in Stager::~Stager' % (path, line(old))]
    old = 'a.persist = flags && persist(mode, a.ncol);'
    assert doctored(old, old + ' (void)hipStreamSynchronize(st.s);') == ['%s:%d: hipStreamSynchronize in cape_pass' % (path, line(old))]
    # an entry point of its own translation unit
    path, src = 'xarray_parcel_amd/csrc/xp_ecape_tu.hip', sources['xarray_parcel_amd/csrc/xp_ecape_tu.hip']
    old = 'launch_columns(k_ncape<decltype(z)>, a.ncol, s, a)'
    assert doctored(old, old.replace(', s, a', ', 0, a')) == ["%s:%d: launch_columns on the default stream ('0')" % (path, line(old))]
    # the launch header itself, and a launcher with a geometry of its own
    for f, old in (('xp_launch.hpp', 'hipLaunchKernelGGL(k, dim3(blocks_for(n)), dim3(256), 0, s, args...)'),
                   ('xp_humidity_tu.hip', 'hipLaunchKernelGGL((k_dewpoint_from<T, KIND(), VEC()>), gr, dim3(256), 0, s, a)')):
        path = 'xarray_parcel_amd/csrc/' + f
        src = sources[path]
        assert doctored(old, old.replace(', 0, s, a', ', 0, 0, a')) == ["%s:%d: hipLaunchKernelGGL on the default stream ('0')" % (path, line(old))]
