"""Compare the gfx950 assembly of one kernel between two builds (the method of profiles/NOTES.md rounds 8 and 10).

  hipcc <the Makefile's flags> -S --cuda-device-only one_instantiation.hip -o a.s        (once per tree)
  isa_compare.py same a.s b.s     instruction streams with symbol names and label numbers masked: IDENTICAL or the first difference
  isa_compare.py table a.s ...    instructions, v_mfma, scratch_*, v_accvgpr_*, VGPRs, AGPRs, s_cbranch, s_barrier, ds_read per file

Each file holds ONE kernel (an explicit instantiation: `template __global__ void tgp::k_rows<7, 4, 1, 10>(tgp::RowArgs);`)."""
import re, sys, hashlib

def load(path):
    """instruction stream of the (single) kernel in a -S file, symbol names and label numbers masked"""
    ins = []
    meta = {}
    inbody = False
    for ln in open(path):
        s = ln.strip()
        m = re.match(r'\.amdhsa_next_free_vgpr (\d+)', s)
        if m: meta['next_free_vgpr'] = int(m.group(1))
        m = re.match(r'\.amdhsa_accum_offset (\d+)', s)
        if m: meta['accum_offset'] = int(m.group(1))
        m = re.match(r'; NumAgprs: (\d+)', s)
        if m: meta['agprs'] = int(m.group(1))
        m = re.match(r'; NumVgprs: (\d+)', s)
        if m: meta['vgprs'] = int(m.group(1))
        m = re.match(r'; ScratchSize: (\d+)', s)
        if m: meta['scratch_bytes'] = int(m.group(1))
        if not s or s.startswith(';') or s.startswith('.') or s.endswith(':'):
            continue
        s = s.split(';')[0].strip()
        s = re.sub(r'_ZN3tgp\w+', 'SYM', s)
        s = re.sub(r'\.LBB\d+_\d+', 'LBL', s)
        ins.append(s)
    return ins, meta

def table(ins, meta):
    c = lambda p: sum(1 for i in ins if re.match(p, i))
    return dict(instructions=len(ins), v_mfma=c(r'v_mfma'), scratch=c(r'scratch_'), accvgpr=c(r'v_accvgpr_'),
                vgprs=meta.get('vgprs'), agprs=meta.get('agprs'), s_cbranch=c(r's_cbranch'), s_barrier=c(r's_barrier'),
                ds_read=c(r'ds_read'), scratch_bytes=meta.get('scratch_bytes'))

if sys.argv[1] == 'same':
    a, ma = load(sys.argv[2]); b, mb = load(sys.argv[3])
    print(sys.argv[2], sys.argv[3], 'IDENTICAL' if a == b else 'DIFFERENT', len(a), len(b),
          hashlib.sha256('\n'.join(a).encode()).hexdigest()[:12], hashlib.sha256('\n'.join(b).encode()).hexdigest()[:12])
    if a != b:
        for k, (x, y) in enumerate(zip(a, b)):
            if x != y:
                print('first difference at', k, '|', x, '|', y); break
else:
    for p in sys.argv[2:]:
        print(p, table(*load(p)))
