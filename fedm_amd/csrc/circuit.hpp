// External circuit of the driven electrodes (include/fedm_hip.h, fedm_circuit_setup / fedm_circuit_measure /
// fedm_circuit_advance / fedm_circuit_get): what the kernels and the C ABI in circuit.hip share with the context's
// teardown.
#pragma once
#include "currents.hpp"

namespace fedm {

// slots of the conductance pass's sums: the pairs g <= h of CUR_MAX potentials, row by row
constexpr int CIRC_SLOTS = CUR_MAX * (CUR_MAX + 1) / 2;
constexpr int circ_slot(int g, int h) { return g * CUR_MAX - g * (g - 1) / 2 + (h - g); }
// fedm_circuit_state.flag
constexpr int CIRC_FLAG_MEASURE = 1, CIRC_FLAG_SINGULAR = 2, CIRC_FLAG_RESULT = 4;

// what lives on the device between the calls: nothing of it is read back unless the caller asks
struct CircState {
    double U[CUR_MAX];                 // the last advance's U^{n+1} (the set-up's U0 before the first)
    double Uo[CUR_MAX], Uo1[CUR_MAX];  // U^n, U^{n-1}: moved by the measure alone
    double cond[CUR_MAX];              // conduction of the measured state [1/s]
    double G[CUR_MAX][CUR_MAX];        // conductance of the measured state [1/(V s)]
    double C[CUR_MAX][CUR_MAX];        // capacitance of the potentials [m]
    double dUdt[CUR_MAX], lead[CUR_MAX];
    int measure_bad, flag;
};

// the advance's arguments, by value
struct CircStep {
    double dt, dt_old;
    double V[CUR_MAX], R[CUR_MAX], Cp[CUR_MAX];
    int n, pad_;
};

struct Circuit {
    int n = 0;
    bool measured = false;
    double R[CUR_MAX] = {}, Cp[CUR_MAX] = {};
    double cap[CUR_MAX][CUR_MAX] = {};   // what CircState::C holds (compared with Currents::cap at every measure)
    CircState *state = nullptr;
    int8_t *entry = nullptr;      // [n_dir] electrode of the context's Dirichlet entry k (through Ctx::dir_perm), -1: none
    // slot-major partials of the conductance pass, one entry per workgroup (postproc.hpp, POST_BLOCKS at the most)
    double *sum_part = nullptr;   // [CIRC_SLOTS][POST_BLOCKS]
    int *flag_part = nullptr;     // [POST_BLOCKS]
};

}  // namespace fedm
