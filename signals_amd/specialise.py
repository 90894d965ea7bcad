"""Run-time specialisation of the two interpreted kernels: voice programs (signals_amd/csrc/voice_program.hip) and block-rate
control programs (control_program.hip).

The interpreter pays for its generality: the dispatch loop carries the whole register file through a `switch`, and the
register allocator copies ~34 doubles per instruction word back into place.  The SAME source built with the
program as a compile-time constant (`-DSIG_VP_STATIC_CODE={...}`) unrolls that loop and folds every switch: straight-line
HIP for exactly one voice graph, 1.6-2x the interpreter's rate.  Control programs likewise, keyed by their STRUCTURE (ops, register
indices, which instructions are wide; `-DSIG_CTL_STATIC_INS / _OUTS`): their registers become VGPRs instead of an LDS file
behind an interpretive loop, 2.3-5x.  This module builds such an image with the ROCm compiler
(`hipcc --genco`, ~3 s; cross-compiles without a GPU), caches it next to the package keyed by the kernel sources and the
build's parameters, and attaches it to the library (`sig_voice_program_attach`), which from then on launches it whenever
`sig_voice_program` is called with that program.  No hipcc, or a failed build: the interpreter keeps running (it is the
same arithmetic; both are checked against the oracle by tests/test_gpu_specialise.py).

Reference semantics are not touched: the image is voice_program.hip itself (same handlers, same block-sequence machine)."""
import hashlib
import os
import pathlib
import re
import shutil
import subprocess
import threading

from . import _native

CSRC = pathlib.Path(__file__).resolve().parent / 'csrc'
CACHE = pathlib.Path(os.environ.get('SIG_SPECIALISE_CACHE') or pathlib.Path(__file__).resolve().parent / '_specialised')
ROOTS = ('voice_program.hip', 'control_program.hip')         # the two files that are built specialised


def _sources() -> tuple:
    """every file a specialised image is compiled from: the two kernels, the closure of their quoted #include "..." lines
    (resolved beside the including file, then in include/), and the public header; paths relative to CSRC, in a fixed order"""
    include = CSRC.parent.parent / 'include'
    seen, todo = {}, [CSRC / name for name in ROOTS] + [include / 'signals_amd.h']
    while todo:
        path = todo.pop().resolve()
        if path in seen:
            continue
        seen[path] = path.read_bytes()
        for name in re.findall(rb'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', seen[path], re.M):
            found = [d / name.decode() for d in (path.parent, include) if (d / name.decode()).exists()]
            if not found:
                raise SpecialiseError(f'{path.name} includes "{name.decode()}", which is neither beside it nor in include/')
            todo.append(found[0])
    return tuple(sorted(os.path.relpath(p, CSRC.resolve()) for p in seen))


_attached: dict = {}        # key -> what attaching returned: True (a voice program), a handle (a control program)
_failed: set = set()
_pending: dict = {}         # key -> the future of its background build
_pool = None                # one worker: builds queue up behind each other
_lock = threading.Lock()


class SpecialiseError(RuntimeError):
    pass


def hipcc() -> str | None:
    found = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    return found if pathlib.Path(found).exists() else None


def _source_digest() -> str:
    h = hashlib.sha1()
    for name in _sources():
        h.update(name.encode() + b'\0' + (CSRC / name).read_bytes())
    return h.hexdigest()


def flags(code: list, n_oscs: int, n_params: int, n_filters: int, n_temps: int, voices_per_lane: int, bus_channels: int) -> list:
    """the macros that make voice_program.hip a kernel for exactly this program: the words, a register file of exactly the
    slots it uses, voices per lane, sink, and the waves per SIMD the interpreter's small build asks for"""
    words = ','.join(f'0x{w:x}' for w in _native.voice_program_words(code))
    ext = int(any(op in _native.VP_EXT_OPS for op, *_ in code))                  # Amp, Adsr, Noise: the extended handlers
    more = ['-DSIG_VP_S_TAB=1'] if any(op in _native.VP_TABLE_OPS for op, *_ in code) else []   # (the tables: a second kernel parameter)
    more += ['-DSIG_VP_S_RES=1'] if any(op in _native.VP_RES_OPS + _native.VP_EQ_OPS for op, *_ in code) else []    # (FilterQ, FilterEq: the resonant design)
    more += ['-DSIG_VP_S_EQ=1'] if any(op in _native.VP_EQ_OPS for op, *_ in code) else []      # (FilterEq: the general numerator on top of it)
    more += ['-DSIG_VP_S_UNI=1'] if any(op in _native.VP_UNI_OPS + _native.VP_BLEP_OPS + _native.VP_SYNC_OPS for op, *_ in code) else []    # (OscUni, OscBlep, OscSync: the copies, a second kernel parameter; run-time values)
    more += ['-DSIG_VP_S_BLEP=1'] if any(op in _native.VP_BLEP_OPS for op, *_ in code) else []   # (OscBlep: the band-limited handler)
    more += ['-DSIG_VP_S_SYNC=1'] if any(op in _native.VP_SYNC_OPS for op, *_ in code) else []   # (OscSync: the hard-sync handler; the ratio is a run-time row)
    # two or more families: the second kernel parameter carries tables and copies together, the kernel has exactly the families of the
    # program.  (Appended last, and only then: the list -- and with it the cache key -- of every other program is what it was)
    more += ['-DSIG_VP_S_MIXED=1'] if len(_native.vp_families(code)) >= 2 else []
    return [f'-DSIG_VP_STATIC_CODE={{{words}}}', f'-DSIG_VP_S_NF={max(n_filters, 1)}', f'-DSIG_VP_S_NO={max(n_oscs, 1)}',
            f'-DSIG_VP_S_NP={max(n_params, 1)}', f'-DSIG_VP_S_NT={n_temps}', f'-DSIG_VP_S_EXT={ext}',
            f'-DSIG_VP_STATIC_VPT={voices_per_lane}', f'-DSIG_VP_STATIC_C={bus_channels}',
            f'-DSIG_VP_STATIC_WAVES={ {1: 3, 2: 2, 4: 1}[voices_per_lane] }'] + more


def _compile(source: str, defs: list, prefix: str) -> bytes:
    """`source` (a file of signals_amd/csrc) built as a gfx950 code object with these macros; cached on disk"""
    key = hashlib.sha1((_source_digest() + source + ' '.join(defs)).encode()).hexdigest()[:24]
    path = CACHE / f'{prefix}_{key}.hsaco'
    if path.exists():
        return path.read_bytes()
    cc = hipcc()
    if cc is None:
        raise SpecialiseError('hipcc not found (set HIPCC): the interpreters keep running')
    try:
        CACHE.mkdir(parents=True, exist_ok=True)
        tmp = path.with_suffix(f'.{os.getpid()}.{threading.get_ident()}.tmp')
        cmd = [cc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-Wno-unused-function', '--genco', *defs,
               '-I', str(CSRC.parent.parent / 'include'), '-o', str(tmp), str(CSRC / source)]
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if done.returncode != 0 or not tmp.exists():
            tmp.unlink(missing_ok=True)
            raise SpecialiseError(f'hipcc failed on the specialised {source}:\n{done.stderr[-2000:]}')
        os.replace(tmp, path)                             # (atomic: another process may be building the same image)
        return path.read_bytes()
    except (OSError, subprocess.TimeoutExpired) as e:     # a read-only package directory, a compiler that cannot be started ...
        raise SpecialiseError(f'specialised {source} not built: {e}') from e


def build(code: list, n_oscs: int, n_params: int, n_filters: int, n_temps: int, voices_per_lane: int, bus_channels: int) -> bytes:
    """the code object (gfx950) of voice_program.hip specialised for this program; cached on disk"""
    return _compile('voice_program.hip', flags(code, n_oscs, n_params, n_filters, n_temps, voices_per_lane, bus_channels), 'vp')


# ---- block-rate control programs (control_program.hip): the same idea, keyed by the program's STRUCTURE (ops, register indices,
# which instructions and outputs are wide); row and output pointers stay run-time arguments
def control_flags(description: list) -> list:
    n_ins, n_outs = description[0], description[1]
    ins = [description[2 + 7 * k: 2 + 7 * k + 7] for k in range(n_ins)]
    outs = [description[2 + 7 * n_ins + 2 * k: 2 + 7 * n_ins + 2 * k + 2] for k in range(n_outs)]
    braces = lambda rows: '{' + ','.join('{' + ','.join(str(int(w)) for w in row) + '}' for row in rows) + '}'
    return [f'-DSIG_CTL_STATIC_INS={braces(ins)}', f'-DSIG_CTL_STATIC_OUTS={braces(outs)}']


# ---- build and attach, once per process and key, for both kinds: `build()` compiles (or loads from the cache), `attach(image)`
# hands the image to the library and returns what the attached kernel is known by
def _ensure(key, what: str, build, attach, background: bool):
    """what `attach` returned for this key, now or earlier; None where it is not available: no hipcc, a failed build (warned
    about once), or -- `background` -- still being built on the worker thread"""
    global _pool
    with _lock:
        if key in _attached:
            return _attached[key]
        if key in _failed or (background and key in _pending):
            return None
        if background:
            if _pool is None:
                import concurrent.futures
                _pool = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix='sig-specialise')
            _pending[key] = _pool.submit(_finish, key, what, build, attach, True)
            return None
    return _finish(key, what, build, attach, False)


def _finish(key, what: str, build, attach, queued: bool):
    try:
        image = build()                                   # (outside the lock: the compiler takes seconds)
        with _lock:
            if key not in _attached:                      # (a synchronous request may have overtaken a queued one)
                _attached[key] = attach(image)
            return _attached[key]
    except (SpecialiseError, _native.NativeError) as e:
        with _lock:
            _failed.add(key)
        import warnings
        warnings.warn(f'{what} not specialised, the interpreter runs it: {e}')
        return None
    finally:
        if queued:
            with _lock:
                _pending.pop(key, None)


def ensure_control(description: list, background: bool = False):
    """the handle of the kernel specialised for this control-program structure (built and attached once per process), or None
    while it is not available (no hipcc, a failed build, or still being built in the background)"""
    key = ('ctl',) + tuple(description)
    with _lock:
        if key not in _attached and key in _pending:      # (being built: the interpreter runs it meanwhile, whoever asks)
            return None
    if description[0] == 0 or description[1] == 0:
        return None
    words = list(description)
    return _ensure(key, 'control program', lambda: _compile('control_program.hip', control_flags(words), 'ctl'),
                   lambda image: _native.control_program_attach(words, image), background)


def _ensure_voice(background: bool, code: list, *sizes) -> bool:
    code = list(code)                                     # (the caller's list may change while a queued build waits)
    got = _ensure(('vp', tuple(code)) + sizes, 'voice program', lambda: build(code, *sizes),
                  lambda image: _native.voice_program_attach(code, *sizes, image) or True, background)
    return got is True


def ensure(code: list, n_oscs: int, n_params: int, n_filters: int, n_temps: int, voices_per_lane: int, bus_channels: int) -> bool:
    """build (or load from the cache) and attach the specialised kernel for this program once per process; False when that is
    not possible here -- the caller's launches then run the interpreter"""
    return _ensure_voice(False, code, n_oscs, n_params, n_filters, n_temps, voices_per_lane, bus_channels)


def ensure_in_background(code: list, n_oscs: int, n_params: int, n_filters: int, n_temps: int, voices_per_lane: int,
                         bus_channels: int) -> bool:
    """`ensure` on a worker thread: True once the kernel is attached, False while it is being built (or cannot be) -- the
    caller's launches run the interpreter until then, so a real-time sink never waits for the compiler"""
    return _ensure_voice(True, code, n_oscs, n_params, n_filters, n_temps, voices_per_lane, bus_channels)


def wait() -> None:
    """block until every background build has finished (tests, benchmarks)"""
    while True:
        with _lock:
            futures = list(_pending.values())
        if not futures:
            return
        for f in futures:
            f.result()


def forget() -> None:
    """detach every specialised voice program (tests); attached control programs keep their handles"""
    wait()
    with _lock:
        _native.voice_program_detach_all()
        for key in [k for k in _attached if k[0] == 'vp']:
            del _attached[key]
        _failed.clear()
