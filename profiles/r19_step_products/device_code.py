"""The gfx950 kernels of two builds of libnavsim_hip.so, compared by name, code size and metadata (registers, LDS, scratch,
kernel-argument size and layout, ...): a change of host launch code must leave all of it as it was.  No GPU needed.

    python profiles/r19_step_products/device_code.py PARENT.so NEW.so

Every object file of the library carries its own code object: the .hip_fatbin section is a row of offload bundles.  Each gfx950
entry is written out, llvm-readelf prints its symbols and its AMDGPU metadata note, and every kernel becomes (object in link order, name) ->
(bytes of code, its metadata entry as text).  Prints one line: kernels in each library, in one only, with another size or metadata.
"""
import os, struct, subprocess, sys, tempfile

import yaml

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib, tmp):
    fat = os.path.join(tmp, "fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "copy")])
    blob = open(fat, "rb").read()
    at = blob.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                yield blob[at + off:at + off + size]
        at = blob.find(MAGIC, at + len(MAGIC))


def kernels(lib):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, elf in enumerate(code_objects(lib, tmp)):
            path = os.path.join(tmp, "co%d" % i)
            open(path, "wb").write(elf)
            sizes = {}
            for line in subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-sW", path], text=True).splitlines():
                f = line.split()
                if len(f) == 8 and f[3] == "FUNC":
                    sizes[f[7]] = int(f[2])
            notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", path], text=True)
            doc = notes[notes.index("---"):notes.rindex("...")]
            for k in yaml.safe_load(doc)["amdhsa.kernels"]:
                out["object %d: %s" % (i, k[".name"])] = (sizes[k[".name"]], yaml.safe_dump(k))
    return out


if __name__ == "__main__":
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only = sorted(set(a) ^ set(b))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print("gfx950 kernels: %d in the parent's library, %d in this one; in one only: %d; same name, other code size or metadata: %d"
          % (len(a), len(b), len(only), len(differ)))
    for k in only + differ:
        print("  ", k[:160])
    sys.exit(1 if only or differ else 0)
