// Host-only driver of contactimplicitmpc/jl_amd/csrc/plant_rollout_call.h (tests/test_plant_rollout_call.py).  One query per input line,
//   check  <entry> key=value ...     -> rc nq nu nc rough      (plant_rollout_check; the model's sizes and `rough` only when rc = 0)
//   layout <entry> key=value ...     -> rc, then `name at n` of every region and `need_* n` of every buffer
// and one output line per query.  <entry> is one of step, step_terrain, rollout, grad, tape, feedback, grad_feedback, tape_feedback and
// fills a PlantRolloutCall the way that entry point of the library does, from a valid hopper_2D call with B = 2, T = 3: u of K_u = 2 rows
// per robot held for 2 steps, w of K_w = 3 shared rows, a mu per robot, n_cols = 2 nq + nu and a schedule of K_f = 2 rows per robot held
// for 2 steps.  key=value lays one thing over that call:
//   an int or a double parameter (B, T, K_u, n_mu, h, reg, K_f, n_sample, opts.max_iter, ...)    a number, hexadecimal floats included
//   a pointer (q0, u, w, mu, opts, q, dz, grad_status, fb, K, x_ref, u_applied, ...)            null
//   K, x_ref                                                                                    v,v,v,...: a heap array of exactly these
//   terrain                                                                                     n:hex, n cimpc_terrain as raw bytes
//   model                                                                                       a CIMPC_PLANT_* id
// Every array the check may read is on the heap at its exact size, so the sanitizer build sees a read past it.
#include "../../contactimplicitmpc/jl_amd/csrc/plant_rollout_call.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

using namespace cimpc;

namespace {

std::vector<double> numbers(const std::string& list) {
    std::vector<double> v;
    std::stringstream ss(list);
    for (std::string item; std::getline(ss, item, ',');) v.push_back(std::strtod(item.c_str(), nullptr));
    return v;
}

// One query's call and the memory it points to
struct Query {
    double dummy[1] = {0.0};      // what the check never reads points here
    int idummy[1] = {0};
    cimpc_ip_opts opts{};
    cimpc_feedback fb{};
    std::vector<double> K, x_ref;
    std::vector<cimpc_terrain> terrain;
    double mu0 = 0.5;
    PlantRolloutCall call{};
    bool ok = true;

    Query(const std::string& entry, const std::map<std::string, std::string>& over) {
        auto has = [&](const char* k) { return over.count(k) != 0; };
        auto num = [&](const char* k, double dflt) { return has(k) ? std::strtod(over.at(k).c_str(), nullptr) : dflt; };
        auto dptr = [&](const char* k) { return has(k) && over.at(k) == "null" ? nullptr : dummy; };
        auto iptr = [&](const char* k) { return has(k) && over.at(k) == "null" ? nullptr : idummy; };
        simulator_opts(&opts);
        for (const auto& [k, v] : over) {
            if (k.rfind("opts.", 0) != 0) continue;
            const std::string f = k.substr(5);
            const double x = std::strtod(v.c_str(), nullptr);
            if (f == "r_tol") opts.r_tol = x; else if (f == "kappa_tol") opts.kappa_tol = x; else if (f == "undercut") opts.undercut = x;
            else if (f == "gamma_reg") opts.gamma_reg = x; else if (f == "kappa_reg") opts.kappa_reg = x; else if (f == "eps_min") opts.eps_min = x;
            else if (f == "ls_scale") opts.ls_scale = x; else if (f == "max_iter") opts.max_iter = (int)x; else if (f == "max_ls") opts.max_ls = (int)x;
            else if (f == "stall_alpha") opts.stall_alpha = x; else if (f == "max_time") opts.max_time = x; else ok = false;
        }
        const bool step = entry == "step" || entry == "step_terrain";
        const bool grad = entry.rfind("grad", 0) == 0, tape = entry.rfind("tape", 0) == 0;
        const bool loop = entry.size() >= 8 && entry.compare(entry.size() - 8, 8, "feedback") == 0;
        if (!step && !grad && !tape && !loop && entry != "rollout") ok = false;
        PlantModel M{};
        const int model = (int)num("model", CIMPC_PLANT_HOPPER_2D);
        if (!plant_model_by_id(model, &M)) M = plant_hopper_2d();      // sizes of the defaults only: the check refuses the id itself
        const int B = (int)num("B", 2), T = (int)num("T", 3);
        if (has("terrain") && over.at("terrain") != "null") {
            const std::string& s = over.at("terrain");
            const size_t colon = s.find(':');
            terrain.resize((size_t)std::atoi(s.c_str()));
            std::vector<unsigned char> bytes;
            for (size_t i = colon + 1; i + 1 < s.size(); i += 2) bytes.push_back((unsigned char)std::strtoul(s.substr(i, 2).c_str(), nullptr, 16));
            if (bytes.size() != terrain.size() * sizeof(cimpc_terrain)) ok = false;
            else if (!terrain.empty()) std::memcpy(terrain.data(), bytes.data(), bytes.size());
        }
        call.model = model; call.B = B;
        call.n_terrain = (int)num("n_terrain", 0);
        call.terrain = terrain.empty() ? nullptr : terrain.data();
        call.needs_terrain = entry == "step_terrain";
        call.q0 = dptr("q0"); call.q1 = dptr("q1");
        call.h = num("h", 0.01);
        call.opts = has("opts") && over.at("opts") == "null" ? nullptr : &opts;
        call.q = dptr("q"); call.gamma = dptr("gamma"); call.b = dptr("b"); call.status = iptr("status"); call.iters = iptr("iters");
        if (step) {      // cimpc_plant_step, cimpc_plant_step_terrain
            call.T = 1; call.steps_per_launch = 1;
            call.u = {dptr("u"), 1, B, 1};
            call.w = {dptr("w"), 1, B, 1};
            call.mu = &mu0; call.n_mu = 1; call.q_row0 = 2;
        } else {
            call.T = T; call.steps_per_launch = (int)num("steps_per_launch", 0);
            call.u = {dptr("u"), (int)num("K_u", 2), (int)num("n_u", B), (int)num("hold_u", 2)};
            call.w = {dptr("w"), (int)num("K_w", 3), (int)num("n_w", 1), (int)num("hold_w", 1)};
            call.mu = dptr("mu"); call.n_mu = (int)num("n_mu", B);
        }
        if (grad || tape)
            call.grad = PlantRolloutGrad{num("reg", 1e-9), (int)num("n_cols", 2 * M.nq + M.nu), dptr("z"), tape ? nullptr : dptr("dz"), iptr("grad_status"), tape};
        if (loop) {
            fb.K_f = (int)num("K_f", 2); fb.n_f = (int)num("n_f", B); fb.hold_f = (int)num("hold_f", 2); fb.n_sample = num("n_sample", 4.0);
            const size_t n_x = (size_t)2 * 2 * 2 * M.nq;      // the default schedule's size, whatever K_f and n_f are laid over it
            K = has("K") && over.at("K") != "null" ? numbers(over.at("K")) : std::vector<double>(n_x * M.nu, 0.0);
            x_ref = has("x_ref") && over.at("x_ref") != "null" ? numbers(over.at("x_ref")) : std::vector<double>(n_x, 0.0);
            fb.K = has("K") && over.at("K") == "null" ? nullptr : K.data();
            fb.x_ref = has("x_ref") && over.at("x_ref") == "null" ? nullptr : x_ref.data();
            call.loop = PlantRolloutLoop{has("fb") && over.at("fb") == "null" ? nullptr : &fb, dptr("u_applied"), dptr("fb_err")};
        }
    }

    // the library's cimpc_default_ip_opts is in cimpc_host.cpp; the simulator's options are what the Python tests pass
    static void simulator_opts(cimpc_ip_opts* o) {
        o->r_tol = 1e-8; o->kappa_tol = 1e-8; o->undercut = INFINITY; o->gamma_reg = 0.1; o->kappa_reg = 0.0; o->eps_min = 0.25;
        o->ls_scale = 0.5; o->max_iter = 100; o->max_ls = 25; o->stall_alpha = 0.0; o->max_time = 0.0;
    }
};

void span(const char* name, const PlantSpan& s) { std::printf(" %s %zu %zu", name, s.at, s.n); }

}  // namespace

int main() {
    for (std::string line; std::getline(std::cin, line);) {
        std::stringstream ss(line);
        std::string what, entry;
        if (!(ss >> what >> entry)) return 1;
        std::map<std::string, std::string> over;
        for (std::string tok; ss >> tok;) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) return 1;
            over[tok.substr(0, eq)] = tok.substr(eq + 1);
        }
        Query Q(entry, over);
        if (!Q.ok) return 1;
        PlantModel M{};
        bool rough = false;
        const int rc = plant_rollout_check(Q.call, &M, &rough);
        if (what == "check") {
            if (rc == CIMPC_OK) std::printf("%d %d %d %d %d\n", rc, M.nq, M.nu, M.nc, rough ? 1 : 0);
            else std::printf("%d\n", rc);
        } else if (what == "layout") {
            std::printf("%d", rc);
            if (rc == CIMPC_OK) {
                const PlantRolloutLayout L = plant_rollout_layout(M, Q.call);
                std::printf(" row %zu TB %zu", L.row, L.TB);
                span("q", L.q); span("u", L.u); span("w", L.w); span("mu", L.mu);
                span("gamma", L.gamma); span("b", L.b); span("status", L.status); span("iters", L.iters); span("z", L.z);
                span("dz", L.dz); span("grad_status", L.grad_status);
                span("fb_K", L.fb_K); span("x_ref", L.x_ref); span("u_applied", L.u_applied); span("fb_err", L.fb_err);
                std::printf(" need_in %zu need_out %zu need_st %zu need_z %zu need_grad %zu need_grad_st %zu need_fb %zu", L.need_in, L.need_out,
                            L.need_st, L.need_z, L.need_grad, L.need_grad_st, L.need_fb);
            }
            std::printf("\n");
        } else {
            return 1;
        }
    }
    return 0;
}
