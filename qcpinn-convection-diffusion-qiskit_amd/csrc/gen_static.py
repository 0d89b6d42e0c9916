"""Generates gen/qc_static_[wave_|h2_]<id>.hip + one gen/qc_static_[wave_|h2_]table.hip per family: compile-time
specialised register-family (n <= 5), lanes-as-amplitudes-family (n = 6..8) and HBM-family (n >= 9) kernels for the gate
programs named below (lowered by ../circuits.py, so the static kernels and the run-time interpreters see the same gate
lists).  Run by the Makefile before compiling."""
import importlib.util
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("qc_circuits", os.path.join(HERE, "..", "circuits.py"))
circuits = importlib.util.module_from_spec(spec)
sys.modules["qc_circuits"] = circuits
spec.loader.exec_module(circuits)

# (ansatz, n_qubits, n_layers, haar)
PROGRAMS = [
    ("cascade", 4, 1, True), ("cascade", 4, 2, True), ("layered", 4, 1, True), ("layered", 4, 2, True),
    ("cross_mesh", 4, 1, True), ("farhi", 4, 1, True), ("sim_circ_15", 4, 1, True), ("cascade", 4, 1, False),
    ("cascade", 5, 1, True), ("alternate", 5, 1, True), ("cascade", 3, 1, False), ("cascade", 2, 1, False),
    (circuits.ROT_RING, 4, 2, False),      # trainer/train.py's Config default (circuits.build_rot_ring_program)
]
# lanes-as-amplitudes family (n = 6..8): (ansatz, n_qubits, n_layers, haar)
WAVE_PROGRAMS = [
    ("layered", 8, 2, True), ("cascade", 6, 1, True), ("cross_mesh", 8, 1, True), ("layered", 7, 1, True),
    ("layered", 6, 1, True), ("layered", 8, 1, True),
]
# HBM family (n >= 9), compile-time stage programs: (ansatz, n_qubits, n_layers, haar, register bits per round).  Two
# entries of one program differ in the tile geometry only; the library takes the first (QC_H2S_RB=3|4 picks by geometry)
H2_PROGRAMS = [
    ("cross_mesh", 16, 1, True, 4), ("cross_mesh", 16, 1, True, 3), ("cross_mesh", 12, 1, True, 4),
    ("cross_mesh", 12, 1, True, 3), ("cross_mesh", 13, 1, True, 4),
]
TWO = (circuits.OP_CNOT, circuits.OP_CRX, circuits.OP_CRZ, circuits.OP_U4)


def lead_rx(rows, n):
    """the leading RX layer folded into the embedding (qc_api.hip, detect_lead_rx)"""
    if len(rows) < n:
        return 0
    for g in range(n):
        op, ba, bb, slot = rows[g]
        if op != circuits.OP_RX or ba != n - 1 - g or slot < 0:
            return 0
    return 1 if len({rows[g][3] for g in range(n)}) == n else 0


def device_rows(prog):
    n = prog.n_qubits
    out = []
    for g in prog.gates:
        ba = n - 1 - g.a
        bb = (n - 1 - g.b) if g.op in TWO else -1
        slot = g.slot if (g.op in circuits.PARAMETRIC or g.op == circuits.OP_U4) else -1
        out.append((g.op, ba, bb, slot))
    return out


def gate_struct(name, n, rows, gate_type, extra=()):
    """the compile-time program of the register and wave families: qubits, gates, (parameters,) gate rows"""
    body = ", ".join("{%d, %d, %d, %d}" % r for r in rows)
    return "\n".join(["namespace {", f"struct {name} {{", f"  static constexpr int N = {n};",
                      f"  static constexpr int G = {len(rows)};", *extra,
                      f"  static constexpr {gate_type} g[{len(rows)}] = {{{body}}};", "};", "}  // namespace"])


def reg_program(i, spec, prog, rows, gates):
    ans, n, L, haar = spec
    return dict(title=f"{ans} n={n} L={L} haar={haar}",
                body=gate_struct(f"SP{i}", n, rows, "SGate", [f"  static constexpr int P = {prog.n_params};"]),
                launch=f"RegLaunch<StatProg<SP{i}>>::table()", table_lines=[], entry=[n, len(rows), gates])


def wave_program(i, spec, prog, rows, gates):
    ans, n, L, haar = spec
    return dict(title=f"wave family, {ans} n={n} L={L} haar={haar}", body=gate_struct(f"WP{i}", n, rows, "WGate"),
                launch=f"WaveLaunch<{n - 4}, StatWave<WP{i}>>::table()", table_lines=[], entry=[n, len(rows), gates])


def h2_plan_tool():
    """the planner itself (qc_hbm2_plan.h, host C++) produces the constexpr plan records of the HBM family"""
    tool = os.path.join(HERE, "gen", "h2_plan_tool")
    deps = [os.path.join(HERE, f) for f in ("h2_plan_tool.cpp", "qc_hbm2_plan.h", "qc_types.h")]
    if not os.path.exists(tool) or any(os.path.getmtime(d) > os.path.getmtime(tool) for d in deps):
        subprocess.run([os.environ.get("HOSTCXX", "g++"), "-O1", "-std=c++17", "-I", HERE, deps[0], "-o", tool], check=True)
    return tool


def h2_program(i, spec, prog, rows, gates):
    ans, n, L, haar, rb = spec
    absorb = lead_rx(rows, n)
    stdin = "\n".join("%d %d %d %d" % r for r in rows) + "\n"
    out = subprocess.run([h2_plan_tool(), f"HP{i}", str(n), str(absorb), str(rb)], input=stdin, capture_output=True,
                         text=True, check=True).stdout
    body, describe = out[:out.index("static const int HP")], out[out.index("static const int HP"):]
    return dict(title=f"HBM family, {ans} n={n} L={L} haar={haar} rb={rb}",
                body="\n".join(["namespace {", body.rstrip(), "}  // namespace"]),
                launch=f"H2sLaunch<HP{i}>::table()", table_lines=[describe.rstrip()],
                entry=[n, len(rows), absorb, rb, gates, f"HP{i}_describe", describe.count(",") + 1])


# per family: file tag, kernel header, launcher record, table entry type and its fields, programs, and the emitter that
# returns one program's title, namespace body, launcher expression, extra table lines and table entry fields
FAMILIES = [
    dict(tag="", header="qc_circuit_reg_kernels.h", launchers="QcRegLaunchers", entry="QcStaticEntry",
         struct="int n_qubits, n_gates; const int* gates; const QcRegLaunchers* launch;", programs=PROGRAMS,
         emit=reg_program),
    dict(tag="wave_", header="qc_circuit_wave_kernels.h", launchers="QcWaveLaunchers", entry="QcStaticWaveEntry",
         struct="int n_qubits, n_gates; const int* gates; const QcWaveLaunchers* launch;", programs=WAVE_PROGRAMS,
         emit=wave_program),
    dict(tag="h2_", header="qc_circuit_h2s_kernels.h", launchers="H2sLaunchers", entry="QcStaticH2Entry",
         struct="int n_qubits, n_gates, absorb, rb; const int* gates; const int* describe; int n_describe; "
                "const H2sLaunchers* launch;", programs=H2_PROGRAMS, emit=h2_program),
]


def lower(spec):
    """the gate program of one (ansatz, n_qubits, n_layers, haar) entry"""
    if spec[0] == circuits.ROT_RING:
        return circuits.build_rot_ring_program(spec[1], spec[2])
    return circuits.build_program(*spec[:4])


def write(path, text):
    if not os.path.exists(path) or open(path).read() != text:
        open(path, "w").write(text)


def main():
    gen = os.path.join(HERE, "gen")
    os.makedirs(gen, exist_ok=True)
    files, tables = [], []
    # one table file per family: the kernel headers are not meant to share a translation unit
    for fam in FAMILIES:
        tag, launchers = fam["tag"], fam["launchers"]
        table = ["// generated by gen_static.py - do not edit", f'#include "../{fam["header"]}"', "",
                 f'struct {fam["entry"]} {{ {fam["struct"]} }};']
        entries = []
        for i, spec in enumerate(fam["programs"]):
            prog = lower(spec)
            rows = device_rows(prog)
            launch, gates = f"qc_static_{tag}launch_{i}", f"qc_static_{tag}gates_{i}"
            p = fam["emit"](i, spec, prog, rows, gates)
            write(os.path.join(gen, f"qc_static_{tag}{i}.hip"),
                  "\n".join([f'// generated by gen_static.py - do not edit: {p["title"]}', f'#include "../{fam["header"]}"',
                             "", p["body"], "", f"extern {launchers} {launch};",
                             f'{launchers} {launch} = {p["launch"]};', ""]))
            files.append(f"gen/qc_static_{tag}{i}.hip")
            flat = ", ".join(str(v) for r in rows for v in r)
            table.append(f"extern {launchers} {launch};")
            table.append(f"static const int {gates}[] = {{{flat}}};")
            table += p["table_lines"]
            entries.append("  {" + ", ".join(str(v) for v in p["entry"] + ["&" + launch]) + "},")
        name = f"qc_static_{tag}table"
        table += [f'extern const {fam["entry"]} {name}[];', f"extern const int qc_static_{tag}count;",
                  f'const {fam["entry"]} {name}[] = {{'] + entries + ["};",
                  f'const int qc_static_{tag}count = {len(fam["programs"])};', ""]
        write(os.path.join(gen, f"{name}.hip"), "\n".join(table))
        tables.append(f"gen/{name}.hip")
    print(" ".join(files + tables))


if __name__ == "__main__":
    main()
