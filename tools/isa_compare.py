"""Are the kernels of a translation unit unchanged, instruction for instruction, after an edit?  Compares two device assembly files
(hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off --cuda-device-only -S file.hip -o file.s, once per source tree) function
by function with local labels renumbered by order of appearance.  Used at the end of round 4 (no GPU time left) to add the
rotated-row / staged training kernel beside k_train_fb / k_train_adam / k_train_fit without touching their measured code:
    python tools/isa_compare.py /tmp/old/train.s /tmp/new/train.s

--by-body: for an edit that changes the kernels' NAMES (a template signature): any number of old files, `--`, any number of new files.
Functions are matched by their normalised body -- a function's own symbol inside it rewritten to a placeholder -- together with the
resource lines of its kernel descriptor (.amdhsa_ registers, scratch, LDS); the two multisets must be equal.  Only text is compared.
    python tools/isa_compare.py --by-body old/a.s old/b.s -- new/a.s new/b.s new/c.s"""
import collections,hashlib,re,sys
def funcs(path):
    out={}; cur=None; buf=[]
    for line in open(path):
        m=re.match(r'^(_Z\w+|k_\w+):\s*(;.*)?$',line)
        if m:
            cur=m.group(1); buf=[]; continue
        if cur is not None:
            if line.startswith('.Lfunc_end'):
                out[cur]=buf; cur=None; continue
            l=line.split(';')[0].rstrip()
            if l.strip(): buf.append(l)
    return out
def norm(buf):
    ids={}
    def sub(m):
        k=m.group(0)
        if k not in ids: ids[k]='L%d'%len(ids)
        return ids[k]
    return [re.sub(r'\.LBB\d+_\d+|\.Lpost_getpc\d+',sub,l) for l in buf]
RESOURCES=('next_free_vgpr','next_free_sgpr','accum_offset','private_segment_fixed_size','group_segment_fixed_size')
def descriptors(path):
    """{kernel: its descriptor's resource lines}"""
    out={}; cur=None
    for line in open(path):
        m=re.match(r'^\s*\.amdhsa_kernel\s+(\S+)',line)
        if m: cur=m.group(1); out[cur]=[]; continue
        if cur is None: continue
        if line.strip().startswith('.end_amdhsa_kernel'): cur=None; continue
        if any('.amdhsa_'+r in line for r in RESOURCES): out[cur].append(' '.join(line.split()))
    return out
def bodies(paths):
    """[(key, name, file)] per kernel: key = hash of the normalised body + descriptor resources"""
    out=[]
    for p in paths:
        d=descriptors(p)
        for k,buf in funcs(p).items():
            if k not in d: continue                      # (a device function that was not inlined: part of no comparison here)
            text='\n'.join(l.replace(k,'<self>') for l in norm(buf))+'\n'+'\n'.join(d[k])
            out.append((hashlib.sha256(text.encode()).hexdigest()[:16],k,p))
    return out
def by_body(old_paths,new_paths):
    o=bodies(old_paths); n=bodies(new_paths)
    co=collections.Counter(k for k,_,_ in o); cn=collections.Counter(k for k,_,_ in n)
    print('kernels: old %d (%d distinct bodies), new %d (%d distinct bodies)'%(len(o),len(co),len(n),len(cn)))
    names_o={k for _,k,_ in o}; names_n={k for _,k,_ in n}
    print('kernels with the same name on both sides: %d'%len(names_o&names_n))
    for key,k,_ in o:
        if k in names_n: print('  by name:',k[:90],'IDENTICAL' if any(key==k2 and k==n2 for k2,n2,_ in n) else 'differs')
    ok=co==cn
    for key in sorted(set(co)|set(cn)):
        if co[key]!=cn[key]:
            print('body %s: old x%d, new x%d'%(key,co[key],cn[key]))
            for kk,k,p in o+n:
                if kk==key: print('   ',p,k[:120])
    print('RESULT:', 'the multisets of kernel bodies and descriptor resources are EQUAL' if ok else 'the multisets DIFFER')
    return 0 if ok else 1
if __name__=='__main__':
    if len(sys.argv)>1 and sys.argv[1]=='--by-body':
        rest=sys.argv[2:]; cut=rest.index('--')
        sys.exit(by_body(rest[:cut],rest[cut+1:]))
    o=funcs(sys.argv[1]); n=funcs(sys.argv[2])
    for k in o:
        a=norm(o[k]); b=norm(n.get(k,[]))
        print(k[:70], len(a), len(b), 'IDENTICAL' if a==b else 'differs')
    for k in n:
        if k not in o: print('new:',k[:70],len(n[k]))
