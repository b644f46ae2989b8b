// census_parity.js — GossipSim.census of ringpop-node_amd/js against the Python binding's
// results for the same scenario (in.json from tests/test_js_census_gpu.py: the cluster, the
// events, and per checked round and observer set the expected census). Prints one JSON line.
'use strict';
var fs = require('fs');
var path = require('path');
var amd = require(path.join(__dirname, '..', '..', 'ringpop-node_amd', 'js'));

var input = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
var fails = [], checks = 0;
var sim = new amd.GossipSim(input.names, {inc0: input.inc0, dead: input.dead, seed: input.seed,
    suspicionRounds: input.suspRounds, now0: input.now0, events: input.events});
var fields = {status: Uint32Array, inRing: Uint32Array, maxInc: Float64Array, atMax: Uint32Array,
    behind: Uint32Array};
input.samples.forEach(function (s) {
    if (s.round > sim.round()) { sim.step(s.round - sim.round()); }
    s.sets.forEach(function (c) {
        var got = sim.census(c.observe === null ? undefined : c.observe);
        checks++;
        if (got.observers !== c.want.observers) { fails.push('round ' + s.round + ' ' + c.name + ' observers'); }
        Object.keys(fields).forEach(function (k) {
            checks++;
            if (!(got[k] instanceof fields[k]) ||
                    JSON.stringify(Array.from(got[k])) !== JSON.stringify(c.want[k])) {
                fails.push('round ' + s.round + ' ' + c.name + ' ' + k);
            }
        });
    });
});
checks++;
try {
    sim.census(new Uint8Array(input.names.length + 1));
    fails.push('a mask of the wrong length was accepted');
} catch (e) {
    if (!(e instanceof TypeError)) { fails.push('wrong-length mask: ' + e); }
}
sim.destroy();
process.stdout.write(JSON.stringify({checks: checks, fails: fails.slice(0, 20), nfail: fails.length}) + '\n');
