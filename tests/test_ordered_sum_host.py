"""One text for the fixed-order sums and for the last-workgroup ticket (csrc/ordered_sum.h), as a property of the
source texts: nothing is compiled and no assembly is read.  A copy of the ticket or of the LDS halving tree that comes back into a
kernel file would have its order of addition, its barriers or its fences kept equal to the header's by hand again."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, '2024-hl-spi3s-sunerf_amd', 'csrc')
HEADER = 'ordered_sum.h'
TICKET_KERNELS = {'train_step.hip': 2, 'likelihood.hip': 1, 'ssim_loss.hip': 1}      # file -> kernels that draw a ticket


def _texts(pattern):
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, pattern)))}


def _code(text):
    """The text without its // comments (the header's comment spells the protocol out)."""
    return re.sub(r'//[^\n]*', '', text)


def _loop_bodies(code):
    """Bodies of the for-loops that halve their counter (``s >>= 1`` in the loop's head), brace-balanced; one statement if unbraced."""
    for m in re.finditer(r'for\s*\([^;{}]*;[^;{}]*;\s*\w+\s*>>=\s*1\s*\)\s*', code):
        at = m.end()
        if code[at] != '{':
            yield code[at:code.index(';', at) + 1]
            continue
        depth, end = 0, at
        while True:
            depth += {'{': 1, '}': -1}.get(code[end], 0)
            end += 1
            if depth == 0:
                break
        yield code[at:end]


def test_the_ticket_is_drawn_in_one_place():
    sources = {**_texts('*.hip'), **_texts('*.h')}
    assert HEADER in sources and len(sources) > 40
    draw = re.compile(r'atomicAdd\s*\(\s*&?\s*\(?[\w.\->]*ticket')
    fence = re.compile(r'__threadfence')
    for name, text in sources.items():
        code = _code(text)
        if name == HEADER:
            assert len(draw.findall(code)) == 1 and len(fence.findall(code)) == 2, 'one draw between the two fences'
            continue
        assert not draw.search(code), f'{name} draws a ticket of its own'
        assert not fence.search(code), f'{name} has a fence of its own: the ticket protocol lives in {HEADER}'
    for name, kernels in TICKET_KERNELS.items():
        code = _code(sources[name])
        assert len(re.findall(r'\blast_block\s*\(', code)) == kernels, name
        assert len(re.findall(r'\.rearm\s*\(\s*\)', code)) == kernels and '.seen()' in code, name
        assert f'#include "{HEADER}"' in code and not re.search(r'\+\s*64\b', code), f'{name} spells the workspace layout out'


def test_no_kernel_file_keeps_a_halving_tree_of_its_own():
    header = _texts(HEADER)[HEADER]
    trees = [b for b in _loop_bodies(_code(header)) if '__syncthreads' in b]
    assert len(trees) == 1 and 'red[k * THREADS + t + s]' in trees[0], 'the header has the one LDS halving tree'
    kept_outside = re.search(r'Kept outside:(.*?)#pragma once', header, re.S).group(1)
    seen = 0
    for name, text in _texts('*.hip').items():
        for body in _loop_bodies(_code(text)):
            seen += 1
            # a halving loop that meets a barrier or stores to an indexed array is a tree through memory; a shuffle loop is neither
            through_memory = '__syncthreads' in body or re.search(r'\w+\s*\[[^\]]*\]\s*(\+|=[^=])', body)
            if through_memory and '__shfl' not in body:
                assert name in kept_outside, f'{name} has a halving tree of its own: {body.strip()[:120]}'
    assert seen >= 5          # the shuffle loops of the render kernels are still found: the search sees halving loops
