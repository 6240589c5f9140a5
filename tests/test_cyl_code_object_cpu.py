"""Code-object checks of the descriptor CNN's fp32 kernel after its bottom map row moved to the direct two-row form
(csrc/convnet_wg.hip, wg_round_direct): everything here is read off the gfx950 code object of the in-tree library, no GPU needed.

* k_cyl_net_wg / k_cyl_net_wg_rerun: no scratch, at most 256 registers of both kinds together (two workgroups per CU), no static LDS
  beside the 80 KB dynamic buffer, no ds_read2_b64 inside a loop, and 38 = 16 + 16 + 6 matrix instructions per (k-step, N-tile) in
  every layer form.
* the cost net's kernel (k_cost_net_w24b) shares wg_pass / wg_round with it and must compile to what it was: its static MFMA count and
  its register and scratch figures are constants read off a build of the commit before the change.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'

# The cost net's kernel pair (csrc/costnet_body.hip: one body for every layer form) in a build of the commit before the two smaller pairs
# were retired (same compiler flags: buffer_amd/build.py; profiles/cost_one_body.md).  mfma: 2 576 in the k-loops + 384 outside.
PARENT_COST_NET = {
    'k_cost_net_w24b': dict(mfma=2960, vgpr=212, agpr=0, scratch=0, sgpr=90),
    'k_cost_net_w24b_rerun': dict(mfma=2960, vgpr=212, agpr=0, scratch=0, sgpr=92),
}


@pytest.fixture(scope='module')
def code_object(tmp_path_factory):
    if not (os.path.exists(f'{LLVM}/llvm-objdump') and os.path.exists(f'{LLVM}/llvm-readelf')):
        pytest.skip('no llvm-objdump / llvm-readelf')
    from buffer_amd import _lib, build
    build.build()
    tmp = tmp_path_factory.mktemp('co')
    so = str(tmp / 'lib.so')
    shutil.copy(_lib.LIB_PATH, so)
    subprocess.run([f'{LLVM}/llvm-objdump', '--offloading', so], capture_output=True, cwd=str(tmp), check=True)
    co = [f for f in os.listdir(tmp) if 'gfx950' in f]
    assert len(co) == 1, os.listdir(tmp)
    asm = subprocess.run([f'{LLVM}/llvm-objdump', '-d', str(tmp / co[0])], capture_output=True, text=True, check=True).stdout
    notes = subprocess.run([f'{LLVM}/llvm-readelf', '--notes', str(tmp / co[0])], capture_output=True, text=True, check=True).stdout
    return asm, notes


def kernel_text(asm, name):
    """[(address, mnemonic, operands and the disassembler's trailing note)] of the kernel `name`"""
    m = re.search(rf'^[0-9a-f]+ <(_Z\d+{name}[A-Z][^>]*)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)', asm, flags=re.S | re.M)
    assert m, name
    out = []
    for ln in m.group(2).splitlines():
        q = re.match(r'\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):(.*)', ln)
        if q:
            out.append((int(q.group(3), 16), q.group(1), q.group(2) + ' ' + q.group(4)))
    assert out, name
    return out


def kernel_meta(notes, name):
    """the kernel's entry of the AMDGPU metadata note as {key: int}"""
    blocks = re.split(r'\n\s+- \.agpr_count:', notes)
    hit = [b for b in blocks[1:] if re.search(rf'\.name:\s+_Z\d+{name}[A-Z]', b)]
    assert len(hit) == 1, (name, len(hit))
    b = '.agpr_count:' + hit[0]
    return {k: int(v) for k, v in re.findall(r'\.(agpr_count|vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|'
                                             r'vgpr_spill_count|sgpr_spill_count):\s+(\d+)', b)}


def loops(text):
    """[(first, last)] instruction indices of the innermost backward branches"""
    addr = {a: i for i, (a, _, _) in enumerate(text)}
    spans = []
    for i, (a, op, args) in enumerate(text):
        if op.startswith('s_cbranch') or op == 's_branch':
            # the disassembler prints the target as '<symbol+0xOFFSET>' behind the encoding
            t = re.search(r'<[^>+]+\+0x([0-9a-f]+)>', args)
            if t:
                target = text[0][0] + int(t.group(1), 16)
                if target <= a and target in addr:
                    spans.append((addr[target], i))
    return [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]


@pytest.mark.parametrize('name', ['k_cyl_net_wg', 'k_cyl_net_wg_rerun'])
def test_cyl_net_resources(code_object, name):
    asm, notes = code_object
    m = kernel_meta(notes, name)
    print(name, m)
    assert m['private_segment_fixed_size'] == 0, 'scratch memory'
    assert m['vgpr_spill_count'] == 0 and m['sgpr_spill_count'] == 0
    # .vgpr_count of the unified file counts both kinds (accumulation registers start at the next multiple of 4 of the VGPRs)
    assert m['vgpr_count'] <= 256 and m['agpr_count'] <= 256
    assert m['group_segment_fixed_size'] == 0, 'static LDS beside the dynamic 80 KB buffer'
    src = open(os.path.join(ROOT, 'buffer_amd', 'csrc', 'convnet_wg.hip')).read()
    maxc, cs = (int(re.search(rf'#define {k} (\d+)', src).group(1)) for k in ('WG_MAXC', 'WG_CS'))
    assert maxc * cs * 4 == 80 * 1024                              # two workgroups in a CU's 160 KB
    text = kernel_text(asm, name)
    assert not [op for _, op, _ in text if re.match(r'v_pk_(mul|add|fma)_f32', op)]
    assert not [op for _, op, _ in text if op.startswith('scratch_')]
    ls = loops(text)
    assert ls, 'no loop found: the disassembly format changed?'
    for a, b in ls:
        bad = [op for _, op, _ in text[a:b + 1] if op == 'ds_read2_b64']
        assert not bad, f'{len(bad)} ds_read2_b64 in the loop at {text[a][0]:#x}'


def test_cyl_net_matrix_instruction_count(code_object):
    """Static count per k-loop (four k-steps per iteration).  A Winograd pass issues 4 components per (k-step, M-tile, N-tile): 64 in the
    128-channel layers (two M-tiles, an N-tile pair), 32 in the others (one M-tile, a pair), four passes per round.  The direct round
    issues 6 per (k-step, N-tile): 48 for the pair, 24 for one N-tile -- 16 + 16 + 6 = 38 per (k-step, N-tile) in every layer form, and
    no loop is left of the two-tap bottom-row form (8 half-empty components: 16 / 32 per loop, two loops per round)."""
    asm, _ = code_object
    text = kernel_text(asm, 'k_cyl_net_wg')
    counts = sorted(sum(1 for _, op, _ in text[a:b + 1] if op.startswith('v_mfma_f32_16x16x4')) for a, b in loops(text))
    counts = [c for c in counts if c]
    print('MFMAs per k-loop of k_cyl_net_wg:', counts)
    # layer forms in the kernel: 128 outputs (pair), 64 outputs (M split), 32 outputs (M and K split; built twice: LDS / global stores)
    assert counts == [24] * 3 + [32] * 12 + [48] + [64] * 4, counts
    assert sum(1 for _, op, _ in text if op.startswith('v_mfma')) == sum(counts)       # none outside the k-loops


@pytest.mark.parametrize('name', sorted(PARENT_COST_NET))
def test_cost_net_compiles_to_what_it_was(code_object, name):
    asm, notes = code_object
    want = PARENT_COST_NET[name]
    m = kernel_meta(notes, name)
    text = kernel_text(asm, name)
    got = dict(mfma=sum(1 for _, op, _ in text if op.startswith('v_mfma')), vgpr=m['vgpr_count'], agpr=m['agpr_count'],
               scratch=m['private_segment_fixed_size'], sgpr=m['sgpr_count'])
    print(name, got)
    assert got == want
