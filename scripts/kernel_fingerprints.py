"""Per-kernel fingerprint of the gfx950 code objects of a built librcot_hip.so (no GPU needed): demangled symbol -> size and sha1
of the function's bytes, and of its 64-byte kernel descriptor (register counts, LDS, scratch) with the code-offset field zeroed.
Two builds whose tables agree on a symbol run the same machine code for it.
  cd BUILD/rcot_amd && /opt/rocm/llvm/bin/llvm-objdump --offloading librcot_hip.so      # writes librcot_hip.so.N.hipv4-...gfx950
  python kernel_fingerprints.py BUILD/rcot_amd > table.txt"""
import hashlib, subprocess, sys, glob, os
RE = "/opt/rocm/llvm/bin/llvm-readelf"
out = {}
for co in sorted(glob.glob(os.path.join(sys.argv[1], "*hipv4-amdgcn-amd-amdhsa--gfx950"))):
    data = open(co, "rb").read()
    secs = {}
    for ln in subprocess.run([RE, "-SW", co], capture_output=True, text=True).stdout.splitlines():
        p = ln.replace("[", " ").replace("]", " ").split()
        if len(p) > 6 and p[0].isdigit():
            secs[int(p[0])] = (int(p[3], 16), int(p[4], 16))        # address, file offset
    for ln in subprocess.run([RE, "-sW", "--demangle", co], capture_output=True, text=True).stdout.splitlines():
        p = ln.split(None, 7)
        if len(p) == 8 and p[3] in ("FUNC", "OBJECT") and p[6].isdigit() and int(p[2]) > 0:
            addr, size, sec = int(p[1], 16), int(p[2]), int(p[6])
            a0, o0 = secs[sec]
            blob = bytearray(data[o0 + addr - a0:o0 + addr - a0 + size])
            if p[7].endswith("(.kd)") and size == 64:
                blob[16:24] = bytes(8)          # kernel_code_entry_byte_offset: where the code sits relative to the descriptor, not what it is
            out.setdefault(p[7], set()).add(f"{size}:{hashlib.sha1(bytes(blob)).hexdigest()[:12]}")
for k in sorted(out):
    print(k, *sorted(out[k]), sep="\t")
