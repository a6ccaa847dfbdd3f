"""Register / LDS / spill report of the product kernels (hipcc -Rpass-analysis=kernel-resource-usage; no GPU needed).
    python tools/kernel_resources.py [source.hip ...] [--filter=substr] [--csrc=DIR] [--text] [--asm-dir=DIR]
--csrc=DIR   compile the sources of another checkout (to compare a parent against a head)
--text       also print each kernel's instruction count and a hash of its gfx950 instruction text (comments, labels' numbers and
             directives left out), so that two builds can be compared kernel by kernel with `diff`
--asm-dir=D  with --text: keep each kernel's instruction text as D/<source>/<mangled name>.s for a closer look at a difference"""
import hashlib, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gst_tacotron_amd", "csrc")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
opt = lambda name: [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--" + name + "=")]
flt = opt("filter")
CSRC = (opt("csrc") or [CSRC])[0]
text = "--text" in sys.argv[1:]
asm_dir = (opt("asm-dir") or [None])[0]
srcs = args or ["skinny_gemm.hip", "dec_front.hip", "gemm_conv.hip", "attention.hip", "gst.hip", "audio.hip"]


def kernel_text(asm):
    """{mangled name: [instruction lines]} of the functions of one device assembly file"""
    out, cur = {}, None
    for ln in asm.splitlines():
        ln = ln.split(";", 1)[0].rstrip()
        m = re.match(r"^([A-Za-z_][\w$.]*):$", ln)
        if m and not m.group(1).startswith(".L"):
            cur = out.setdefault(m.group(1), [])
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
        s = ln.strip()
        if cur is None or not s or s.startswith("."):       # directives and local labels
            continue
        cur.append(re.sub(r"\.LBB\d+_\d+", ".LBB", s))
    return out


for src in srcs:
    with tempfile.TemporaryDirectory() as td:
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-c",
               os.path.join(CSRC, src), "-o", os.path.join(td, "o.o"), "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        body = {}
        if text:
            s = os.path.join(td, "o.s")
            subprocess.run(cmd[:7] + ["--cuda-device-only", "-S", cmd[8], "-o", s], capture_output=True, text=True, check=True)
            body = kernel_text(open(s).read())
    cur = None
    rows = {}
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", ln)
        if m:
            cur = m.group(1); rows[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+)", ln)
        if m and cur:
            rows[cur][m.group(1).strip()] = m.group(2)
    for name, v in rows.items():
        dn = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        if flt and not any(f in dn for f in flt):
            continue
        tail = ""
        if text:
            lines = body.get(name, [])
            tail = " insts %5d text %s" % (len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()[:12])
            if asm_dir:
                os.makedirs(os.path.join(asm_dir, src), exist_ok=True)
                with open(os.path.join(asm_dir, src, name[:150] + "." + hashlib.sha256(name.encode()).hexdigest()[:8] + ".s"), "w") as f:
                    f.write("\n".join(lines) + "\n")
        print("%-100s VGPR %3s AGPR %3s SGPR %3s spill %3s sspill %3s scratch %4s occ %2s LDS %6s%s" % (dn[:100], v.get("VGPRs"), v.get("AGPRs"),
              v.get("TotalSGPRs"), v.get("VGPRs Spill"), v.get("SGPRs Spill"), v.get("ScratchSize [bytes/lane]"), v.get("Occupancy [waves/SIMD]"),
              v.get("LDS Size [bytes/block]"), tail))
