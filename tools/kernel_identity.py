#!/usr/bin/env python3
"""Is the gfx950 device code of this tree byte-identical to revision REV's?

Builds kernels/*.hip of both trees with build_native's command line and
tools/microbench/gemm_loop.hip device-only in its three forms, unbundles the
gfx950 ELF of each and compares bytes: per file ``identical`` or the kernels
whose bytes differ; a file REV does not have is reported as ``new``.  Exit
status 1 on any difference.  No instruction is
inspected.  Usage: python tools/kernel_identity.py REV [NEW=OLD ...]

A kernel that grows, arrives or leaves moves the kernels after it, and a
kernel descriptor (``NAME.kd``) holds the distance to its code: the per-kernel
comparison leaves those eight bytes out, so a kernel is listed only when its
code or the rest of its descriptor changed.  ``NEW=OLD`` compares this tree's
kernel NEW (code and descriptor) with REV's kernel OLD, in every file that has
both: ``256x256pb0=256x256pb`` shows that a reference tile is the kernel REV
shipped under the other name.
"""
import concurrent.futures as cf, hashlib, io, os, shutil, struct, subprocess, sys, tarfile, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cekirdekler_amd import build_native as bn  # noqa: E402

KREL, MREL = "cekirdekler_amd/kernels", "tools/microbench"
PROBES = {"gemm_loop": [], "gemm_loop_l2": ["-DCEK_PROBE_L2"], "gemm_loop_ts": ["-DCEK_PROBE_TS"]}


def device_elfs(tree: str) -> dict:
    """name -> bytes of the unbundled gfx950 ELF, for every build of `tree`.

    Compiled from inside `tree` with relative paths: hipcc hashes the paths it
    is given into a symbol name (__hip_cuid_*), so two trees compare equal
    only when their command lines are spelled alike."""
    os.makedirs(os.path.join(tree, "out"))
    rel = lambda cmd: [a.replace(tree + os.sep, "") for a in cmd]
    cmds = {f[:-4]: rel(bn.kernel_command(os.path.join(tree, KREL, f), os.path.join("out", f[:-4] + ".co")))
            for f in sorted(os.listdir(os.path.join(tree, KREL))) if f.endswith(".hip")}
    for name, defs in PROBES.items():
        cmds[name] = [bn.hipcc_path(), "--genco", f"--offload-arch={bn.ARCH}", "-O3", "-std=c++17", *defs,
                      os.path.join(MREL, "gemm_loop.hip"), "-o", os.path.join("out", name + ".co")]

    def build(cmd: list) -> bytes:
        for c in (cmd, [os.path.join(bn.ROCM, "llvm", "bin", "clang-offload-bundler"), "--type=o", "--unbundle",
                        f"--targets=hipv4-amdgcn-amd-amdhsa--{bn.ARCH}", f"--input={cmd[-1]}", f"--output={cmd[-1]}.elf"]):
            r = subprocess.run(c, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode:
                sys.exit(" ".join(c) + "\n" + r.stdout)
        return open(os.path.join(tree, cmd[-1] + ".elf"), "rb").read()

    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        return dict(zip(cmds, ex.map(build, cmds.values())))


def symbols(elf: bytes) -> dict:
    """name -> bytes of every sized symbol of an ELF64 (kernels and their descriptors)."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for s in sec:
        if s[1] != 2:  # SHT_SYMTAB
            continue
        stroff = sec[s[6]][4]
        for o in range(s[4], s[4] + s[5], 24):
            name, _info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, o)
            if size and 0 < shndx < shnum and sec[shndx][1] != 8:  # not SHT_NOBITS
                at = sec[shndx][4] + value - sec[shndx][3]
                out[elf[stroff + name:elf.index(b"\0", stroff + name)].decode()] = elf[at:at + size]
    return out


def placed(sym: dict) -> dict:
    """The symbols with every descriptor's offset to its code (bytes 16-23 of the 64) zeroed."""
    return {k: v[:16] + bytes(8) + v[24:] if k.endswith(".kd") and len(v) == 64 else v for k, v in sym.items()}


def main() -> int:
    rev = sys.argv[1]
    pairs = [a.split("=") for a in sys.argv[2:]]
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, KREL, MREL], check=True, stdout=subprocess.PIPE).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(os.path.join(tmp, "rev"))
        for d in (KREL, MREL):  # this tree's sources, to the same depth as REV's
            shutil.copytree(os.path.join(ROOT, d), os.path.join(tmp, "cur", d),
                            ignore=lambda _d, fs: [f for f in fs if not f.endswith((".hip", ".h"))])
        old, new = device_elfs(os.path.join(tmp, "rev")), device_elfs(os.path.join(tmp, "cur"))
    bad = 0
    for name in sorted(set(old) | set(new)):
        a, b = old.get(name, b""), new.get(name, b"")
        if name not in old:  # a file this tree adds: nothing to be identical to
            print(f"{name}: new  sha256 {hashlib.sha256(b).hexdigest()}")
            continue
        if a == b:
            print(f"{name}: identical  sha256 {hashlib.sha256(a).hexdigest()}")
            continue
        sha = " -> ".join(hashlib.sha256(x).hexdigest()[:16] for x in (a, b))
        bad += 1
        sa, sb = (placed(symbols(x)) if x else {} for x in (a, b))
        diff = sorted(k for k in set(sa) | set(sb) if sa.get(k) != sb.get(k))
        print(f"{name}: DIFFERENT  sha256 {sha}\n  " + ("\n  ".join(diff) or "(outside every sized symbol)"))
        for new_k, old_k in pairs:
            hit = [s for s in sb if s.endswith("_" + new_k) and s[:-len(new_k)] + old_k in sa]
            for s in hit:
                o = s[:-len(new_k)] + old_k
                same = sb[s] == sa[o] and sb[s + ".kd"] == sa[o + ".kd"]
                print(f"  {s}: {'identical to' if same else 'DIFFERENT from'} {rev}'s {o}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
