"""No build-time switches in the kernels, as a property of the source texts: nothing is compiled.  A variant
that was measured and not adopted is removed and stays in the commit that measured it (tools/experiments/README.md); the only
preprocessor conditional left in csrc/ separates hipcc from a plain host compiler.  A tool or a test that still passes one of
the project's switches to the build would silently build the shipped kernel and report it as a variant."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc')
ALLOWED = {'__HIPCC__'}      # sunerf_common.h, prep_math.h: headers that a host-only compiler reads too

CONDITIONAL = re.compile(r'^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b([^\n]*)', re.M)
SWITCH_FLAG = re.compile(r'-D[ \t]?((?:SUNERF|PIPE)_\w+)')      # the project's prefixes (a test of build.sh's pass-through may say -DEXTRA)


def _tested_names():
    """file -> the identifiers its preprocessor conditionals test."""
    tested = {}
    for path in sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h'))):
        code = re.sub(r'//[^\n]*', '', open(path).read())
        names = set()
        for m in CONDITIONAL.finditer(code):
            names |= set(re.findall(r'[A-Za-z_]\w*', m.group(1))) - {'defined'}
        if names:
            tested[os.path.basename(path)] = names
    return tested


def test_the_only_preprocessor_conditionals_separate_hipcc_from_a_host_compiler():
    tested = _tested_names()
    assert len(glob.glob(os.path.join(CSRC, '*.hip'))) > 30 and ALLOWED <= set().union(*tested.values())
    switches = {name: sorted(names - ALLOWED) for name, names in tested.items() if names - ALLOWED}
    assert not switches, f'build-time switches: {switches}'


def test_no_tool_and_no_test_passes_a_switch_that_the_kernels_do_not_test():
    tested = set().union(*_tested_names().values())
    files = [p for p in glob.glob(os.path.join(ROOT, 'tools', '**', '*'), recursive=True)
             if os.path.isfile(p) and os.sep + 'experiments' + os.sep not in p]      # tools/experiments: records of their commits
    files += glob.glob(os.path.join(ROOT, 'tests', '*.py'))
    assert len(files) > 100
    stale = {}
    for path in files:
        try:
            text = open(path, encoding='utf-8').read()
        except UnicodeDecodeError:      # a probe's binary built next to its source
            continue
        names = set(SWITCH_FLAG.findall(text)) - tested
        if names:
            stale[os.path.relpath(path, ROOT)] = sorted(names)
    assert not stale, f'flags that build nothing: {stale}'
